// Arithmetic shared by the stencil kernels, no kernel itself: jac and its vector
// forms, the lane-crossing moves, the rotated-pair fp32 and wide-lane fp64
// register layouts with their Body* structs, and the strip geometry.
#pragma once

#include <hip/hip_runtime.h>

#include "mxs/kernels/kernels.hpp"

namespace mxs::kernels::detail {

template <typename T>
struct Vec16 {
  static constexpr int N = 16 / sizeof(T);
  using type = T __attribute__((ext_vector_type(N)));
};

template <typename T>
__device__ __forceinline__ T fma_t(T a, T b, T c);
template <>
__device__ __forceinline__ float fma_t<float>(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
template <>
__device__ __forceinline__ double fma_t<double>(double a, double b, double c) { return __builtin_fma(a, b, c); }

// One output cell, fixed evaluation order (see kernels.hpp).
template <typename T>
__device__ __forceinline__ T jac(T c, T n, T s, T w, T e, T c0, T c1) {
  return fma_t<T>(c1, (n + s) + (w + e), c0 * c);
}

// Coefficient sources of the level loops. A uniform pass hands the kernels its
// two scalars; a level-table pass (Chebyshev relaxation, mxs/kernels/relaxation.hpp)
// its table, passed by value in the kernel arguments. The level loops ask
// level_coeff(c, l), in the pipeline with l a compile-time constant once they
// are unrolled, so a table entry is a scalar load from the kernel-argument
// segment and a uniform coefficient the scalar it always was. LevelArray: one
// array per coefficient (the held tile indexes it at run time).
template <typename T, int S>
struct LevelArray {
  T v[S];
};
template <typename T>
__device__ __forceinline__ T level_coeff(T c, int) {
  return c;
}
template <typename T, int S>
__device__ __forceinline__ T level_coeff(const LevelArray<T, S>& c, int l) {
  return c.v[l];
}
// The pipeline's level source: (c0, c1) of a level side by side, so a level is
// one aligned SGPR pair (one s_load_dwordx2 / x4) that both the multiply and the
// FMA of a level read (stencil_pipe_levels.hpp: BodyRotLevelsF32). The level
// bodies take the pair as their coefficient argument.
template <typename T>
struct alignas(2 * sizeof(T)) CoeffPair {
  T c0, c1;
};
template <typename T, int S>
struct LevelPairs {
  CoeffPair<T> v[S];
};
template <typename T, int S>
__device__ __forceinline__ CoeffPair<T> level_coeff(const LevelPairs<T, S>& c, int l) {
  return c.v[l];
}
// A level source may also carry a correction tile that the pipeline adds to
// every stored cell (the source term, stencil_pipe_levels.hpp). The
// pipeline asks CoeffCorr<C>::value at compile time, so the kernels of every
// other coefficient source keep their instructions.
template <typename C>
struct CoeffCorr {
  static constexpr bool value = false;
};
template <typename T, int S>
struct LevelPairsSrc {
  LevelPairs<T, S> pairs;
  const T* corr;  // a tile of the pass's geometry; only core cells are read
};
template <typename T, int S>
struct CoeffCorr<LevelPairsSrc<T, S>> {
  static constexpr bool value = true;
};
template <typename T, int S>
__device__ __forceinline__ CoeffPair<T> level_coeff(const LevelPairsSrc<T, S>& c, int l) {
  return c.pairs.v[l];
}
template <typename C>
__device__ __forceinline__ const void* coeff_corr(const C&) {
  return nullptr;
}
template <typename T, int S>
__device__ __forceinline__ const T* coeff_corr(const LevelPairsSrc<T, S>& c) {
  return c.corr;
}

constexpr int kWavesPerBlock = 4;
constexpr int kNumXcds = 8;  // MI355X: workgroups are dealt round-robin over 8 XCDs
constexpr int kBlock = kWavesPerBlock * kWaveSize;

// One vector of outputs from its three rows and the two scalars beside `mid`.
template <typename T, typename V, int N>
__device__ __forceinline__ V jac_vec(const V& up, const V& mid, const V& dn, T left, T right, T c0, T c1) {
  V o;
  o[0] = jac<T>(mid[0], up[0], dn[0], left, mid[1 % N], c0, c1);
  if constexpr (N == 2) {
    o[1] = jac<T>(mid[1], up[1], dn[1], mid[0], right, c0, c1);
  } else {
#pragma unroll
    for (int q = 1; q < N - 1; ++q) o[q] = jac<T>(mid[q], up[q], dn[q], mid[q - 1], mid[q + 1], c0, c1);
    o[N - 1] = jac<T>(mid[N - 1], up[N - 1], dn[N - 1], mid[N - 2], right, c0, c1);
  }
  return o;
}

// fp32 x4 form written on aligned register pairs, so the backend emits packed
// v_pk_{add,mul,fma}_f32 without pair-building moves; the horizontal sums are
// scalar adds written straight into pairs. Same per-element operations and
// order as jac() (IEEE add is commutative), so results are bitwise identical.
using f32x2 = float __attribute__((ext_vector_type(2)));
using f32x4 = float __attribute__((ext_vector_type(4)));
__device__ __forceinline__ f32x4 jac_vec4f(const f32x4& up, const f32x4& mid, const f32x4& dn, float left,
                                           float right, float c0, float c1) {
  const f32x2 ns_lo = up.xy + dn.xy, ns_hi = up.zw + dn.zw;
  f32x2 we_lo, we_hi;
  we_lo.x = left + mid.y;
  we_lo.y = mid.x + mid.z;
  we_hi.x = mid.y + mid.w;
  we_hi.y = mid.z + right;
  const f32x2 c0v = f32x2(c0), c1v = f32x2(c1);
  const f32x2 lo = __builtin_elementwise_fma(c1v, ns_lo + we_lo, c0v * mid.xy);
  const f32x2 hi = __builtin_elementwise_fma(c1v, ns_hi + we_hi, c0v * mid.zw);
  f32x4 o;
  o.xy = lo;
  o.zw = hi;
  return o;
}

template <typename T, typename V>
__device__ __forceinline__ V jac_row(const V& up, const V& mid, const V& dn, T left, T right, T c0, T c1) {
  if constexpr (sizeof(T) == 4) return jac_vec4f(up, mid, dn, left, right, c0, c1);
  else return jac_vec<T, V, Vec16<T>::N>(up, mid, dn, left, right, c0, c1);
}

template <typename T>
__device__ __forceinline__ T lane_fetch(T v, int byte_addr);
template <>
__device__ __forceinline__ float lane_fetch<float>(float v, int a) {
  return __int_as_float(__builtin_amdgcn_ds_bpermute(a, __float_as_int(v)));
}
template <>
__device__ __forceinline__ double lane_fetch<double>(double v, int a) {
  const long long b = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_ds_bpermute(a, int(b & 0xffffffff));
  const int hi = __builtin_amdgcn_ds_bpermute(a, int(b >> 32));
  return __longlong_as_double((static_cast<long long>(hi) << 32) | static_cast<unsigned int>(lo));
}

// Whole-wavefront DPP shifts (CDNA keeps the GFX9 wave_shr / wave_shl controls):
// lane i reads lane i-1 (kDppWaveShr1) or lane i+1 (kDppWaveShl1); the shifted-in
// lane gets 0. As a DPP source modifier the shift folds into the consuming
// v_add_f32, so a column neighbour costs no instruction and no LDS round trip.
constexpr int kDppWaveShl1 = 0x130;
constexpr int kDppWaveShr1 = 0x138;
template <typename T, int CTRL>
__device__ __forceinline__ T lane_shift(T v);
template <>
__device__ __forceinline__ float lane_shift<float, kDppWaveShr1>(float v) {
  return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), kDppWaveShr1, 0xf, 0xf, true));
}
template <>
__device__ __forceinline__ float lane_shift<float, kDppWaveShl1>(float v) {
  return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), kDppWaveShl1, 0xf, 0xf, true));
}
// 64-bit DPP takes no wave shifts: two dword moves. bound_ctrl zero-fills the
// shifted-in lane (0.0), so no zeroed `old` register (one v_mov each) is needed.
template <>
__device__ __forceinline__ double lane_shift<double, kDppWaveShr1>(double v) {
  const long long b = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_mov_dpp(int(b & 0xffffffff), kDppWaveShr1, 0xf, 0xf, true);
  const int hi = __builtin_amdgcn_mov_dpp(int(b >> 32), kDppWaveShr1, 0xf, 0xf, true);
  return __longlong_as_double((static_cast<long long>(hi) << 32) | static_cast<unsigned int>(lo));
}
template <>
__device__ __forceinline__ double lane_shift<double, kDppWaveShl1>(double v) {
  const long long b = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_mov_dpp(int(b & 0xffffffff), kDppWaveShl1, 0xf, 0xf, true);
  const int hi = __builtin_amdgcn_mov_dpp(int(b >> 32), kDppWaveShl1, 0xf, 0xf, true);
  return __longlong_as_double((static_cast<long long>(hi) << 32) | static_cast<unsigned int>(lo));
}

// ------------------------------------------------ rotated-pair fp32 layout
// Measured on the S = 16 stream kernel (scripts/isa_mix.py): with the natural
// register layout (c0 c1 | c2 c3) the horizontal sums (c[i-1] + c[i+1]) straddle
// the 64-bit pairs the packed VALU works on, so the backend builds pairs with 4
// v_mov_b32 and keeps 2 v_mov_b32_dpp: 18 VALU issue slots per level-row, ~75
// cycles at one wave per SIMD. Holding every intermediate row ROTATED as
// A = (c1, c2), B = (c3, c0) makes the in-lane pair (c0 + c2, c3 + c1) one
// v_pk_add_f32 with swapped halves (op_sel), and the two lane-crossing sums
// c2 + c0[lane+1], c1 + c3[lane-1] two v_add_f32 with a DPP wave shift folded
// into the source, written straight into the pair (we3, we0) that lines up with
// B. Per level-row: 9 packed + 2 DPP adds, no moves. Same operations, same
// operand order per cell as jac() (IEEE add is commutative): bitwise identical.
// Only the input rows (natural order from HBM) and the stored top level are
// rotated, once per row each.
__device__ __forceinline__ f32x4 rot_in(const f32x4& n) { return __builtin_shufflevector(n, n, 1, 2, 3, 0); }
__device__ __forceinline__ f32x4 rot_out(const f32x4& r) { return __builtin_shufflevector(r, r, 3, 0, 1, 2); }
// rot_in as two v_pk_mov_b32 into fresh registers. From the shufflevector the
// backend often keeps the rotated row as halves of the loaded registers (the
// op_sel of later adds reads them in place), so the next load into that
// prefetch slot needs other registers and the loop back edge copies them back:
// ~21 v_mov per 6 rows of the fetching stage, plus 4 v_mov instead of 2
// v_pk_mov for some rotations (ISA of the S = 20 pipeline). Copying here ends
// the loaded registers' lifetime at the rotation.
__device__ __forceinline__ f32x4 rot_in_copy(const f32x4& n) {
  const f32x2 lo = n.xy, hi = n.zw;
  f32x2 a, b;
  asm("v_pk_mov_b32 %0, %1, %2 op_sel:[1,0]" : "=v"(a) : "v"(lo), "v"(hi));  // (c1, c2)
  asm("v_pk_mov_b32 %0, %1, %2 op_sel:[1,0]" : "=v"(b) : "v"(hi), "v"(lo));  // (c3, c0)
  return __builtin_shufflevector(a, b, 0, 1, 2, 3);
}

__device__ __forceinline__ f32x4 jac_rot4f(const f32x4& up, const f32x4& mid, const f32x4& dn, float c0, float c1) {
  const f32x2 am = mid.xy, bm = mid.zw;  // (c1, c2), (c3, c0)
  const f32x2 ns_a = up.xy + dn.xy, ns_b = up.zw + dn.zw;
  const f32x2 we_a = bm.yx + am.yx;  // (c0 + c2, c3 + c1)
  f32x2 we_b;
  we_b.x = __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(bm.y), kDppWaveShl1, 0xf, 0xf, true)) + am.y;
  we_b.y = __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(bm.x), kDppWaveShr1, 0xf, 0xf, true)) + am.x;
  const f32x2 c0v = f32x2(c0), c1v = f32x2(c1);
  const f32x2 oa = __builtin_elementwise_fma(c1v, ns_a + we_a, c0v * am);
  const f32x2 ob = __builtin_elementwise_fma(c1v, ns_b + we_b, c0v * bm);
  f32x4 o;
  o.xy = oa;
  o.zw = ob;
  return o;
}

template <typename T, int S>
struct StreamShape {
  static constexpr int N = Vec16<T>::N;
  static constexpr int SA = ((S + N - 1) / N) * N;      // apron columns per side
  static constexpr int OW = kWaveSize * N - 2 * SA;     // output columns per wave
};

// ------------------------------------------------ wide-lane fp64 layout
// fp64 has no packed VALU and 64-bit DPP cannot take the wave shifts, so the
// natural fp64 form (one 16-byte vector = 2 cells per lane, 128-column strips)
// pays 2 neighbour moves (4 v_mov_b32_dpp) per 2 cells and an apron of 2S of
// 128 columns. Four cells per lane (two 16-byte loads, 256-column strips as
// fp32) halve both: 20 fp64 ops + 4 dword moves per 4 cells, apron 2S of 256.
// Same per-cell operations and order as jac(): bitwise identical.
using f64x2 = double __attribute__((ext_vector_type(2)));
using f64x4 = double __attribute__((ext_vector_type(4)));
// The loaded row into fresh registers (4 v_mov_b64): as rot_in_copy for fp32,
// this ends the prefetch registers' lifetime at entry, so the next load can
// reuse them instead of the loop back edge copying rows around.
__device__ __forceinline__ f64x4 copy_w4d(const f64x4& v) {
  f64x4 r;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    double x;
    asm("v_mov_b64 %0, %1" : "=v"(x) : "v"(v[i]));
    r[i] = x;
  }
  return r;
}
__device__ __forceinline__ f64x4 jac_w4d(const f64x4& up, const f64x4& mid, const f64x4& dn, double c0, double c1) {
  const double left = lane_shift<double, kDppWaveShr1>(mid.w);   // lane - 1's last cell
  const double right = lane_shift<double, kDppWaveShl1>(mid.x);  // lane + 1's first cell
  f64x4 o;
  o.x = jac<double>(mid.x, up.x, dn.x, left, mid.y, c0, c1);
  o.y = jac<double>(mid.y, up.y, dn.y, mid.x, mid.z, c0, c1);
  o.z = jac<double>(mid.z, up.z, dn.z, mid.y, mid.w, c0, c1);
  o.w = jac<double>(mid.w, up.w, dn.w, mid.z, right, c0, c1);
  return o;
}

// Per-lane bodies of the branch-free streaming kernels (stream_chunk_fast,
// pipe_chunk): 4 cells per lane in both, so a strip is 256 columns and the
// apron S rounded up to 4. `enter` maps a row loaded from HBM into the
// register layout the levels work on; `store` maps it back and writes one
// lane's 4 cells through the chunk's buffer descriptor (an offset past the
// range is dropped by the hardware range check: no branch, no exec mask).
using u32x4 = unsigned __attribute__((ext_vector_type(4)));
struct BodyRotF32 {  // rotated-pair fp32 (jac_rot4f)
  using T = float;
  using V = f32x4;
  static constexpr int N = 4;
  // A scheduling fence after each row iteration of the pipeline's fetching
  // stage (pipe_chunk): keeps the scheduler from overlapping consecutive rows'
  // level chains, which holds more rows live (see BodySumF64).
  static constexpr bool kStage0Fence = false;
  static __device__ __forceinline__ V zero() { return f32x4(0.f); }
  static __device__ __forceinline__ V load(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
  static __device__ __forceinline__ V enter(const V& v) { return rot_in_copy(v); }
  static __device__ __forceinline__ V jac(const V& u, const V& m, const V& d, float c0, float c1) {
    return jac_rot4f(u, m, d, c0, c1);
  }
  static __device__ __forceinline__ void store(const V& top, __amdgpu_buffer_rsrc_t r, unsigned off, float) {
    const f32x4 nat = rot_out(top);
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, nat), r, int(off), 0, 2 /* nt */);
  }
};
struct BodyWideF64 {  // 4 consecutive fp64 cells per lane (jac_w4d)
  using T = double;
  using V = f64x4;
  static constexpr int N = 4;
  static constexpr bool kStage0Fence = false;  // see BodyRotF32
  static __device__ __forceinline__ V zero() { return f64x4(0.0); }
  static __device__ __forceinline__ V load(const double* p) {
    const f64x2 a = *reinterpret_cast<const f64x2*>(p), b = *reinterpret_cast<const f64x2*>(p + 2);
    return __builtin_shufflevector(a, b, 0, 1, 2, 3);
  }
  static __device__ __forceinline__ V enter(const V& v) { return copy_w4d(v); }
  static __device__ __forceinline__ V jac(const V& u, const V& m, const V& d, double c0, double c1) {
    return jac_w4d(u, m, d, c0, c1);
  }
  static __device__ __forceinline__ void store(const V& top, __amdgpu_buffer_rsrc_t r, unsigned off, double) {
    const f64x2 lo = top.xy, hi = top.zw;
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, lo), r, int(off), 0, 2 /* nt */);
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, hi), r, int(off + 16u), 0, 2 /* nt */);
  }
};

// A lane's 4 cells of a correction tile (CoeffCorr), loaded through a buffer
// descriptor laid over it like the output's and at the store's own offset: a
// dropped lane or row is past the range and loads 0. The add is one rounded
// operation per cell, in natural cell order (after rot_out for the rotated
// fp32 layout), then the store of the body.
template <typename T>
struct CorrRow {
  u32x4 v[sizeof(T) / 4];
};
__device__ __forceinline__ void corr_load(CorrRow<float>& c, __amdgpu_buffer_rsrc_t r, unsigned off) {
  c.v[0] = __builtin_amdgcn_raw_buffer_load_b128(r, int(off), 0, 0);
}
__device__ __forceinline__ void corr_load(CorrRow<double>& c, __amdgpu_buffer_rsrc_t r, unsigned off) {
  c.v[0] = __builtin_amdgcn_raw_buffer_load_b128(r, int(off), 0, 0);
  c.v[1] = __builtin_amdgcn_raw_buffer_load_b128(r, int(off + 16u), 0, 0);
}
__device__ __forceinline__ void corr_store(const f32x4& top, const CorrRow<float>& c, __amdgpu_buffer_rsrc_t r,
                                           unsigned off) {
  const f32x4 nat = rot_out(top) + __builtin_bit_cast(f32x4, c.v[0]);
  __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, nat), r, int(off), 0, 2 /* nt */);
}
__device__ __forceinline__ void corr_store(const f64x4& top, const CorrRow<double>& c, __amdgpu_buffer_rsrc_t r,
                                           unsigned off) {
  const f64x2 lo = top.xy + __builtin_bit_cast(f64x2, c.v[0]), hi = top.zw + __builtin_bit_cast(f64x2, c.v[1]);
  __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, lo), r, int(off), 0, 2 /* nt */);
  __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, hi), r, int(off + 16u), 0, 2 /* nt */);
}

// Sum form (c_center == c_neighbor == c, the default 5-point average). The
// S-level recurrence u' = c * (5-point sum of u) is linear with one uniform
// scale, so a pass carries v_l = u_l / c^l — plain 5-point sums, no multiply —
// and applies c^S once when it stores (the kernels' c0 argument holds c^S).
// The horizontal 3-sums come from pair sums: with p = u[2k] + u[2k+1],
// h3(x) = p(x) + u[x even ? x - 1 : x + 1]. Rotated fp32: 8 VALU issue slots
// per 4 cells and level instead of 11 (2 ns + 1 pair + 1 + 2 DPP h3 + 2 sum);
// wide fp64: 14 fp64 ops + 4 moves instead of 20 + 4. The result equals the
// step-by-step evaluation up to rounding (not bit for bit: different
// association, one scale per pass instead of one per step); magnitudes grow
// as 5^S inside a pass (|u| up to 3e38 / 5^S stays finite).
// (a.x + b.y, a.y + b.x): one v_pk_add_f32 with the halves of src1 swapped by
// op_sel. Written as asm so the swap is never materialised as a register pair
// of its own (from a shufflevector the backend copies swapped pairs with
// v_mov_b32: ~1 per level-row of the sum body, measured in the ISA). Plain
// VALU, no hazard the compiler would have to know about.
__device__ __forceinline__ f32x2 pk_add_swap(const f32x2& a, const f32x2& b) {
  f32x2 r;
  asm("v_pk_add_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,0]" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
__device__ __forceinline__ f32x4 sum_rot4f(const f32x4& up, const f32x4& mid, const f32x4& dn) {
  const f32x2 am = mid.xy, bm = mid.zw;  // (c1, c2), (c3, c0)
  const f32x2 ns_a = up.xy + dn.xy, ns_b = up.zw + dn.zw;
  const f32x2 p = pk_add_swap(am, bm);   // (c1 + c0, c2 + c3)
  const f32x2 h_a = pk_add_swap(p, am);  // (p01 + c2, p23 + c1) = h3(c1), h3(c2)
  f32x2 h_b;                             // h3(c3) = c4 + p23, h3(c0) = c[-1] + p01
  h_b.x = __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(bm.y), kDppWaveShl1, 0xf, 0xf, true)) + p.y;
  h_b.y = __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(bm.x), kDppWaveShr1, 0xf, 0xf, true)) + p.x;
  f32x4 o;
  o.xy = ns_a + h_a;
  o.zw = ns_b + h_b;
#ifdef MXS_TEST_VALU_PAD
  // Test builds only (tests/test_gpu_cycles.py, profiles/r06_cycles): one more
  // VALU slot per level-row (9 instead of 8, +12.5%), results unchanged (x * 1).
  float pad = o.x;
  asm volatile("v_mul_f32 %0, 1.0, %0" : "+v"(pad));
  o.x = pad;
#endif
  return o;
}
__device__ __forceinline__ f64x4 sum_w4d(const f64x4& up, const f64x4& mid, const f64x4& dn) {
  const double left = lane_shift<double, kDppWaveShr1>(mid.w);
  const double right = lane_shift<double, kDppWaveShl1>(mid.x);
  const double p01 = mid.x + mid.y, p23 = mid.z + mid.w;
  f64x4 o;
  o.x = (up.x + dn.x) + (p01 + left);
  o.y = (up.y + dn.y) + (p01 + mid.z);
  o.z = (up.z + dn.z) + (p23 + mid.y);
  o.w = (up.w + dn.w) + (p23 + right);
  return o;
}
struct BodySumF32 : BodyRotF32 {
  static __device__ __forceinline__ V jac(const V& u, const V& m, const V& d, float, float) { return sum_rot4f(u, m, d); }
  static __device__ __forceinline__ void store(const V& top, __amdgpu_buffer_rsrc_t r, unsigned off, float scale) {
    BodyRotF32::store(top * scale, r, off, scale);
  }
};
struct BodySumF64 : BodyWideF64 {
  // Without the fence the ascending 8 + 8 pass (fp64 8192^2) needs more than
  // the 256 VGPRs two waves per SIMD allow and spills 44 B per lane to
  // scratch; fenced: 231 VGPRs, no scratch, 1.5% faster (profiles/r06_fp64).
  static constexpr bool kStage0Fence = true;
  static __device__ __forceinline__ V jac(const V& u, const V& m, const V& d, double, double) { return sum_w4d(u, m, d); }
  static __device__ __forceinline__ void store(const V& top, __amdgpu_buffer_rsrc_t r, unsigned off, double scale) {
    BodyWideF64::store(top * scale, r, off, scale);
  }
};

// Scaled form (any c_center, c_neighbor != 0; the fp32 pipeline and balanced
// stream kernels, the fp64 wide pipeline at depth 16). The update is this framework's (the reference's
// Compute() is empty: stencil2d/mpi-2d-stencil-subarray-cuda.cu:32-37; SURVEY
// K10). u' = c1 (N + S + W + E + k u) with k = c0 / c1, so a pass
// carries v_l = u_l / c1^l, v' = (N + S + W + E) + k v — one packed FMA per
// cell pair in place of the per-step form's multiply and FMA — and applies c1^S
// once when it stores (the kernels' c0 argument holds c1^S, their c1 argument
// k). Rotated fp32: 9 VALU issue slots per 4 cells and level instead of 11;
// wide fp64: 16 fp64 ops + 4 moves instead of 20 + 4. The sum form is the
// k = 1 case with the centre folded into the horizontal pair sums (8 slots).
// Equal to the per-step evaluation up to rounding; magnitudes grow as
// (4 + |k|)^S inside a pass (the solver's range guard).
__device__ __forceinline__ f32x4 scaled_rot4f(const f32x4& up, const f32x4& mid, const f32x4& dn, float k) {
  const f32x2 am = mid.xy, bm = mid.zw;  // (c1, c2), (c3, c0)
  const f32x2 ns_a = up.xy + dn.xy, ns_b = up.zw + dn.zw;
  const f32x2 we = am + bm;                 // (c1 + c3, c2 + c0): the in-lane neighbour pairs, swapped
  const f32x2 t_a = pk_add_swap(ns_a, we);  // (ns(c1) + c0 + c2, ns(c2) + c1 + c3)
  f32x2 we_b;                               // c3: c2 + c0[lane + 1], c0: c1 + c3[lane - 1]
  we_b.x = __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(bm.y), kDppWaveShl1, 0xf, 0xf, true)) + am.y;
  we_b.y = __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(bm.x), kDppWaveShr1, 0xf, 0xf, true)) + am.x;
  const f32x2 kv = f32x2(k);
  f32x4 o;
  o.xy = __builtin_elementwise_fma(kv, am, t_a);
  o.zw = __builtin_elementwise_fma(kv, bm, ns_b + we_b);
  return o;
}
__device__ __forceinline__ f64x4 scaled_w4d(const f64x4& up, const f64x4& mid, const f64x4& dn, double k) {
  const double left = lane_shift<double, kDppWaveShr1>(mid.w);
  const double right = lane_shift<double, kDppWaveShl1>(mid.x);
  f64x4 o;
  o.x = __builtin_fma(k, mid.x, (up.x + dn.x) + (left + mid.y));
  o.y = __builtin_fma(k, mid.y, (up.y + dn.y) + (mid.x + mid.z));
  o.z = __builtin_fma(k, mid.z, (up.z + dn.z) + (mid.y + mid.w));
  o.w = __builtin_fma(k, mid.w, (up.w + dn.w) + (mid.z + right));
  return o;
}
struct BodyScaledF32 : BodyRotF32 {
  static __device__ __forceinline__ V jac(const V& u, const V& m, const V& d, float, float k) {
    return scaled_rot4f(u, m, d, k);
  }
  static __device__ __forceinline__ void store(const V& top, __amdgpu_buffer_rsrc_t r, unsigned off, float scale) {
    BodyRotF32::store(top * scale, r, off, scale);
  }
};
struct BodyScaledF64 : BodyWideF64 {
  static __device__ __forceinline__ V jac(const V& u, const V& m, const V& d, double, double k) {
    return scaled_w4d(u, m, d, k);
  }
  static __device__ __forceinline__ void store(const V& top, __amdgpu_buffer_rsrc_t r, unsigned off, double scale) {
    BodyWideF64::store(top * scale, r, off, scale);
  }
};

// XB: alternative bodies. The tuner specialises FastBody<T, SUM, 1>
// (bench/tune_kernels.hpp); the library uses XB = 0 and, with SUM, the scaled
// form as XB = kScaledBody.
constexpr int kScaledBody = 2;
template <typename T, bool SUM = false, int XB = 0>
struct FastBody;
template <>
struct FastBody<float, true, kScaledBody> {
  using type = BodyScaledF32;
};
template <>
struct FastBody<double, true, kScaledBody> {
  using type = BodyScaledF64;
};
template <>
struct FastBody<float, false, 0> {
  using type = BodyRotF32;
};
template <>
struct FastBody<double, false, 0> {
  using type = BodyWideF64;
};
template <>
struct FastBody<float, true, 0> {
  using type = BodySumF32;
};
template <>
struct FastBody<double, true, 0> {
  using type = BodySumF64;
};

// Strip geometry of the kernels: FAST = the 4-cells-per-lane bodies above,
// else one 16-byte vector per lane (StreamShape). Identical for fp32.
template <typename T, int S, bool FAST>
struct StripShape {
  static constexpr int N = FAST ? 4 : Vec16<T>::N;
  static constexpr int SA = ((S + N - 1) / N) * N;
  static constexpr int OW = kWaveSize * N - 2 * SA;
};

}  // namespace mxs::kernels::detail
