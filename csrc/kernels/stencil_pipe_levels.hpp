// The two-stage pipeline with a level table (Chebyshev relaxation,
// mxs/kernels/relaxation.hpp): pipe_chunk of stencil_pipe_kernels.hpp in
// the per-step form, ghost-ring tiles only (no wrap), with one coefficient pair
// per level instead of two uniforms. Same forms as the uniform per-step pass
// (pipe_form_for(..., EvalForm::PerStep, ...), with_pipe_form), same shares,
// same VALU work per cell.
//
// One kernel and one launcher for both level sources C (stencil_bodies.hpp):
// LevelPairs<T, S>, the table alone ("stream_pipe_levels"), and
// LevelPairsSrc<T, S>, the table and `corr`, a tile of the pass's geometry (the
// source term, docs/ARCHITECTURE.md "Source term": "stream_pipe_levels_src").
// With the latter, stage 1 of pipe_chunk loads a lane's 4 cells of `corr` at
// the store's own offset when it starts a row's level chain and adds them to the
// row it stores (CoeffCorr): one more read stream over the core and one rounded
// add per cell, every level untouched. Only cells that are stored are read from
// `corr` (a dropped lane or row is past the descriptor's range and loads 0), so
// its ghost ring and padding never enter.
// Instantiated in stencil_pipe_levels_f32.hip (S = 20, 24) and
// stencil_pipe_levels_f64.hip (S = 12, 16), with `corr` in
// stencil_pipe_levels_src_f32.hip and stencil_pipe_levels_src_f64.hip, so the
// translation units of the uniform kernels compile as before.
#pragma once

#include "mxs/kernels/relaxation.hpp"
#include "stencil_pipe.hpp"

namespace mxs {
namespace kernels {
namespace detail {

// The per-step bodies with a level's (c0, c1) in ONE aligned SGPR pair. The
// packed fp32 math reads a 64-bit scalar operand per instruction; from two
// separate scalars the backend keeps every coefficient as a splat pair (c, c),
// 4 SGPRs per level, and a 12-level stage then spills SGPRs to VGPR lanes
// (v_readlane in the row loop: 1200-4100 per kernel at 8 + 12 .. 12 + 12).
// Here the multiply broadcasts the pair's low half and the FMA its high half
// through op_sel, 2 SGPRs per level. The same v_pk_mul_f32 / v_pk_fma_f32 per
// cell pair as jac_rot4f, so results are bitwise those of the uniform kernels.
__device__ __forceinline__ f32x4 jac_rot4f_pair(const f32x4& up, const f32x4& mid, const f32x4& dn, const f32x2 cc) {
  const f32x2 am = mid.xy, bm = mid.zw;  // (c1, c2), (c3, c0)
  const f32x2 ns_a = up.xy + dn.xy, ns_b = up.zw + dn.zw;
  const f32x2 we_a = bm.yx + am.yx;  // (c0 + c2, c3 + c1)
  f32x2 we_b;
  we_b.x = __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(bm.y), kDppWaveShl1, 0xf, 0xf, true)) + am.y;
  we_b.y = __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(bm.x), kDppWaveShr1, 0xf, 0xf, true)) + am.x;
  const f32x2 sa = ns_a + we_a, sb = ns_b + we_b;
  f32x2 pa, pb, oa, ob;
  asm("v_pk_mul_f32 %0, %1, %2 op_sel_hi:[0,1]" : "=v"(pa) : "s"(cc), "v"(am));  // c0 * centre
  asm("v_pk_mul_f32 %0, %1, %2 op_sel_hi:[0,1]" : "=v"(pb) : "s"(cc), "v"(bm));
  asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[1,0,0] op_sel_hi:[1,1,1]" : "=v"(oa) : "s"(cc), "v"(sa), "v"(pa));  // c1 * sums + it
  asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[1,0,0] op_sel_hi:[1,1,1]" : "=v"(ob) : "s"(cc), "v"(sb), "v"(pb));
  f32x4 o;
  o.xy = oa;
  o.zw = ob;
  return o;
}
struct BodyRotLevelsF32 : BodyRotF32 {
  static __device__ __forceinline__ V jac(const V& u, const V& m, const V& d, CoeffPair<float> p, CoeffPair<float>) {
    f32x2 cc;
    cc.x = p.c0;
    cc.y = p.c1;
    return jac_rot4f_pair(u, m, d, cc);
  }
  static __device__ __forceinline__ void store(const V& top, __amdgpu_buffer_rsrc_t r, unsigned off, CoeffPair<float>) {
    BodyRotF32::store(top, r, off, 0.f);
  }
};
struct BodyWideLevelsF64 : BodyWideF64 {  // fp64 has no packed math: the pair is two scalars
  static __device__ __forceinline__ V jac(const V& u, const V& m, const V& d, CoeffPair<double> p, CoeffPair<double>) {
    return jac_w4d(u, m, d, p.c0, p.c1);
  }
  static __device__ __forceinline__ void store(const V& top, __amdgpu_buffer_rsrc_t r, unsigned off, CoeffPair<double>) {
    BodyWideF64::store(top, r, off, 0.0);
  }
};
template <typename T>
struct LevelBody;
template <>
struct LevelBody<float> {
  using type = BodyRotLevelsF32;
};
template <>
struct LevelBody<double> {
  using type = BodyWideLevelsF64;
};

// The table rides in the kernel arguments (2 S scalars behind the 2 KB of
// PipeShares): every level's pair is a scalar load, nothing is stored.
template <int S0, int S1, int PF, typename T, bool JOINT, int LAG1, typename C>
__global__ __launch_bounds__(2 * kWavesPerBlock * kWaveSize) void stencil5_stream_pipe_levels_kernel(
    const T* __restrict__ in, T* __restrict__ out, index_t pitch, index_t core_off, index_t W, index_t H,
    index_t x_begin, index_t x_end, index_t y_begin, index_t y_end, const PipeShares shares, const C cs) {
  // The share walk of stencil5_stream_pipe_kernel (no wrap, no tuning switches),
  // over a level source: see the note at the top of stencil_pipe_kernels.hpp.
  constexpr int G = kWavesPerBlock;
  using P = PipeShape<S0, S1, PF>;
  using B = typename LevelBody<T>::type;
  constexpr int OW = StripShape<T, P::S, true>::OW;
  constexpr int OWG = JointShape<S0, S1, G>::OWG;
  __shared__ typename B::V ring[G * P::RING * kWaveSize];
  const index_t rows = y_end - y_begin;
  const index_t strips = (x_end - x_begin + OW - 1) / OW;
  const index_t groups = JOINT ? (x_end - x_begin + OWG - 1) / OWG : (strips + G - 1) / G;
  constexpr bool SPLIT = pipe_split_form<T, S0, S1, G, JOINT, LAG1>();
  const index_t half = SPLIT ? shares.split_half : 0;
  const index_t total = half > 0 ? (groups - 1) * rows + half : groups * rows;
  const int wave = threadIdx.x / kWaveSize;
  const int strip = wave % G, stage = wave / G;
  const index_t slot = blockIdx.x;
  index_t a, b;
  if (shares.n > 0) {
    a = shares.start[slot];
    b = shares.start[slot + 1];
  } else {
    a = slot * shares.share;
    b = a + shares.share < total ? a + shares.share : total;
  }
  const index_t max_rows = kMaxChunkBytes / (pitch * index_t(sizeof(T)));
  if (max_rows < 1) return;  // workgroup-uniform, before any barrier (never launched so: the host checks)
#pragma unroll 1
  while (a < b) {  // workgroup-uniform: all 8 waves take every chunk (barriers inside)
    const index_t grp = a / rows, r0 = a - grp * rows;
    if constexpr (SPLIT) {
      if (half > 0 && grp == groups - 1) {  // the split narrow group, as in stencil5_stream_pipe_kernel
        index_t r1 = half < r0 + (b - a) ? half : r0 + (b - a);
        r1 = r1 - r0 > max_rows ? r0 + max_rows : r1;
        const int sub = wave_uniform(strip / 2), sstrip = wave_uniform(strip % 2);
        const index_t q0 = wave_uniform(!sub ? r0 : r0 + half < rows ? r0 + half : rows);
        const index_t q1 = wave_uniform(!sub ? r1 : r1 + half < rows ? r1 + half : rows);
        using J = JointShape<S0, S1, G>;
        pipe_chunk<B, S0, S1, PF, false, true, G, LAG1, true, 0u>(in, out, pitch, core_off, W, H, x_begin + grp * OWG,
                                                                 x_end, y_begin + q0, y_begin + q1, cs, cs,
                                                                 ring + sub * (J::ROW / 2), stage, sstrip, r1 - r0, G / 2);
        a += r1 - r0;
        continue;
      }
    }
    index_t r1 = rows < r0 + (b - a) ? rows : r0 + (b - a);
    r1 = r1 - r0 > max_rows ? r0 + max_rows : r1;
    if constexpr (JOINT) {
      pipe_chunk<B, S0, S1, PF, false, true, G, LAG1, false, 0u>(in, out, pitch, core_off, W, H, x_begin + grp * OWG,
                                                                x_end, y_begin + r0, y_begin + r1, cs, cs, ring, stage,
                                                                strip);
    } else {
      const index_t xw = x_begin + (grp * G + strip) * OW;
      pipe_chunk<B, S0, S1, PF, false, false, G, LAG1, false, 0u>(in, out, pitch, core_off, W, H, xw, x_end, y_begin + r0,
                                                                 y_begin + r1, cs, cs,
                                                                 ring + strip * P::RING * kWaveSize, stage);
    }
    a += r1 - r0;
  }
}

// `cs`: the filled level source; `name`: the dispatch name of its launches.
template <typename T, int S, int JS0, int LAG1, typename C>
void launch_pipe_levels_form(const T* in, T* out, const TileGeom& g, index_t x0, index_t x1, index_t y0, index_t y1,
                             const C& cs, const char* name, const PipeChoice& ch, hipStream_t s) {
  constexpr PipeForm P = kPerStrip<T, S, EvalForm::PerStep>;
  constexpr int S0 = JS0 > 0 ? JS0 : P.s0;
  constexpr auto kernel = stencil5_stream_pipe_levels_kernel<S0, S - S0, P.pf, T, (JS0 > 0), (JS0 > 0 ? LAG1 : 0), C>;
  const int blocks = resident_workgroups(reinterpret_cast<const void*>(kernel), 2 * kBlock, 1);
  const PipeShares shares =
      pipe_pass_shares<T>("stencil5_tb_levels", g, ch, x1 - x0, y1 - y0, blocks,
                          pipe_split_form<T, JS0, S - JS0, kWavesPerBlock, (JS0 > 0), LAG1>());
  kernel<<<blocks, 2 * kBlock, 0, s>>>(in, out, g.pitch, g.core_offset(), g.width, g.height, x0, x1, y0, y1, shares, cs);
  note_launch(name, ch.form, shares.split_half > 0, false);
}

// One S-level pass over [x0, x1) x [y0, y1) of a ghost-ring tile in the form
// the uniform per-step pass of these columns takes.
template <typename T, int S, typename C>
void launch_pipe_levels_impl(const T* in, T* out, const TileGeom& g, index_t x0, index_t x1, index_t y0, index_t y1,
                             const C& cs, const char* name, hipStream_t s) {
  const PipeChoice ch = pipe_form_for(int(sizeof(T)), S, EvalForm::PerStep, x1 - x0, pipe_switches());
  with_pipe_form<T, S, EvalForm::PerStep>(ch, [&](auto tag) {
    using K = decltype(tag);
    launch_pipe_levels_form<T, S, K::JS0, K::LAG1>(in, out, g, x0, x1, y0, y1, cs, name, ch, s);
  });
}

// Explicitly instantiated in the four level-pipeline TUs, each for its source.
template <typename T, int S, typename C>
void launch_pipe_levels(const T* in, T* out, const TileGeom& g, index_t x0, index_t x1, index_t y0, index_t y1,
                        const C& cs, const char* name, hipStream_t s);
#define MXS_INST_PIPE_LEVELS(T, S, C)                                                                                 \
  template void launch_pipe_levels<T, S, C<T, S>>(const T*, T*, const TileGeom&, index_t, index_t, index_t, index_t, \
                                                  const C<T, S>&, const char*, hipStream_t)

}  // namespace detail
}  // namespace kernels
}  // namespace mxs
