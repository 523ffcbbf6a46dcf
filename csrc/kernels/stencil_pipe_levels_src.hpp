// The level-table pipeline with a correction tile (the source term,
// docs/ARCHITECTURE.md "Source term"): stencil5_stream_pipe_levels_kernel of
// stencil_pipe_levels.hpp whose coefficient source also carries `corr`, a tile
// of the pass's geometry. Stage 1 of pipe_chunk loads a lane's 4 cells of
// `corr` at the store's own offset when it starts a row's level chain and adds
// them to the row it stores (CoeffCorr, stencil_bodies.hpp): one more read
// stream over the core and one rounded add per cell, every level untouched.
// Only cells that are stored are read from `corr` (a dropped lane or row is
// past the descriptor's range and loads 0), so its ghost ring and padding never
// enter. Same forms, shares and launch shape as the pass without `corr`.
// Instantiated in stencil_pipe_levels_src_f32.hip (S = 20, 24) and
// stencil_pipe_levels_src_f64.hip (S = 12, 16).
#pragma once

#include "stencil_pipe_levels.hpp"

namespace mxs {
namespace kernels {
namespace detail {

template <int S0, int S1, int PF, typename T, bool JOINT, int LAG1>
__global__ __launch_bounds__(2 * kWavesPerBlock * kWaveSize) void stencil5_stream_pipe_levels_src_kernel(
    const T* __restrict__ in, T* __restrict__ out, index_t pitch, index_t core_off, index_t W, index_t H,
    index_t x_begin, index_t x_end, index_t y_begin, index_t y_end, const PipeShares shares,
    const LevelPairsSrc<T, S0 + S1> cs) {
  // The share walk of stencil5_stream_pipe_levels_kernel, written out again:
  // see the note at the top of stencil_pipe_kernels.hpp.
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

template <typename T, int S, int JS0, int LAG1>
void launch_pipe_levels_src_form(const T* in, T* out, const TileGeom& g, index_t x0, index_t x1, index_t y0, index_t y1,
                                 const LevelTable& t, const T* corr, const PipeChoice& ch, hipStream_t s) {
  constexpr PipeForm P = kPerStrip<T, S, EvalForm::PerStep>;
  constexpr int S0 = JS0 > 0 ? JS0 : P.s0;
  constexpr auto kernel =
      stencil5_stream_pipe_levels_src_kernel<S0, S - S0, P.pf, T, (JS0 > 0), (JS0 > 0 ? LAG1 : 0)>;
  // Shares exactly as launch_pipe_levels_form computes them.
  const index_t rows = y1 - y0, groups = pipe_groups(ch.form, x1 - x0);
  const index_t split_half = pipe_split_half(ch, x1 - x0, rows);
  MXS_CHECK(split_half == 0 || (pipe_split_form<T, JS0, S - JS0, kWavesPerBlock, (JS0 > 0), LAG1>()),
            "stencil5_tb_levels: this pipeline form does not split its last group");
  const int blocks = resident_workgroups(reinterpret_cast<const void*>(kernel), 2 * kBlock, 1);
  const index_t total = split_half > 0 ? (groups - 1) * rows + split_half : groups * rows;
  PipeShares shares = PipeShares::equal((total + blocks - 1) / blocks);
  shares.split_half = split_half;
  if (pipe_balanced() && blocks <= kMaxShareBlocks)
    pipe_starts(groups, rows, blocks, pipe_fill_rows(ch.form), &shares, split_half);
  MXS_CHECK(chunk_rows_fit(g.pitch, sizeof(T)),
            "stencil5_tb_levels: rows of " << g.pitch * index_t(sizeof(T)) << " bytes leave fewer than " << kMinChunkRows
                                           << " rows per pipeline chunk (buffer-descriptor stores)");
  LevelPairsSrc<T, S> cs;
  cs.pairs = level_pairs<T, S>(t);
  cs.corr = corr;
  kernel<<<blocks, 2 * kBlock, 0, s>>>(in, out, g.pitch, g.core_offset(), g.width, g.height, x0, x1, y0, y1, shares, cs);
  note_launch("stream_pipe_levels_src", ch.form, split_half > 0, false);
}

template <typename T, int S>
void launch_pipe_levels_src_impl(const T* in, T* out, const TileGeom& g, index_t x0, index_t x1, index_t y0, index_t y1,
                                 const LevelTable& t, const T* corr, hipStream_t s) {
  const PipeChoice ch = pipe_form_for(int(sizeof(T)), S, EvalForm::PerStep, x1 - x0, pipe_switches());
  with_pipe_form<T, S, EvalForm::PerStep>(ch, [&](auto tag) {
    using K = decltype(tag);
    launch_pipe_levels_src_form<T, S, K::JS0, K::LAG1>(in, out, g, x0, x1, y0, y1, t, corr, ch, s);
  });
}

// Explicitly instantiated in the two source-term pipeline TUs.
template <typename T, int S>
void launch_pipe_levels_src(const T* in, T* out, const TileGeom& g, index_t x0, index_t x1, index_t y0, index_t y1,
                            const LevelTable& t, const T* corr, hipStream_t s);

}  // namespace detail
}  // namespace kernels
}  // namespace mxs
