// Two-stage pipeline launchers (stencil_pipe_kernels.hpp: stencil5_stream_pipe_kernel),
// compiled in their own translation units (stencil_pipe_f32.hip,
// stencil_pipe_f64.hip: ~100 kernel instantiations) and called by the shape
// dispatch in stencil.hip. The form of a pass is chosen by pipe_form_for()
// (mxs/kernels/pipe_form.hpp) for the one-launch pass here and the chunk-list
// pass (stencil_pipe_chunks.hip) alike; with_pipe_form() maps it to the kernel
// instantiations for both.
#pragma once

#include <algorithm>
#include <cmath>

#include "mxs/core/error.hpp"
#include "mxs/kernels/kernels.hpp"
#include "mxs/runtime/hip_utils.hpp"
#include "stencil_pipe_kernels.hpp"

namespace mxs {
namespace kernels {
namespace detail {

static_assert(kPipeStrips == kWavesPerBlock, "pipe_form.hpp counts the strips of a pipeline workgroup");
static_assert(eval_xb(EvalForm::Scaled) == kScaledBody && eval_xb(EvalForm::Sum) == 0, "EvalForm -> <SUM, XB>");

// stencil.hip: the record behind last_stencil_dispatch() / last_pipe_form().
void note_launch(const char* kernel, const PipeForm& form = {}, bool split = false, bool block_prio = false);

// Workgroups of `kernel` (at `threads` per workgroup) resident at once on this
// device, occupancy (at least min_per_cu) x CUs, over the processes sharing the
// GPU (gpu_share()). The occupancy query is memoised per kernel.
int resident_workgroups(const void* kernel, int threads, int min_per_cu);

// fp64 depths the wide-lane pipeline takes (S0 = S/2, S1 = S - S0 <= 8 levels
// per stage: the windows fit 2 waves/SIMD without spilling).
constexpr int kPipeMinF64 = 9;

// What the kernels take as (c0, c1): per step the coefficients, sum form
// (c^S, c), scaled form (c1^S, k = c0 / c1). k is formed from the element-type
// coefficients: the one-launch and the chunk-list pass run the same k, so they
// stay bitwise equal.
template <typename T>
struct KernelCoeffs {
  T a, b;
};
template <typename T>
KernelCoeffs<T> kernel_coeffs(EvalForm f, T c0, T c1, int S) {
  if (f == EvalForm::PerStep) return {c0, c1};
  return {T(std::pow(double(c1), double(S))), f == EvalForm::Scaled ? T(double(c0) / double(c1)) : c1};
}

// A compile-time pipeline form: JS0 = 0 the per-strip layout, else joint
// windows with S0 = JS0; LAG1 the level-order mask; EF the evaluation form.
template <int JS0_, int LAG1_, EvalForm EF_>
struct PipeTag {
  static constexpr int JS0 = JS0_, LAG1 = LAG1_;
  static constexpr EvalForm EF = EF_;
};
template <typename T, int S, EvalForm EF>
constexpr PipeForm kPerStrip = pipe_form_for(int(sizeof(T)), S, EF, 0, {false, false, false}).form;

// The instantiation table of both launcher families: calls fn(PipeTag) for the
// compile-time form equal to `c`. The candidates are every choice
// pipe_form_for() can make for <T, S, EF> — all switches on below and from
// kJointWide columns, ascending order off, joint windows off — so the kernels
// instantiated are exactly the forms the rule can pick; any other form fails.
template <typename T, int S, EvalForm EF, int I = 0, typename F>
void with_pipe_form(const PipeChoice& c, F&& fn) {
  if constexpr (I < 4) {
    constexpr PipeChoice k = pipe_form_for(int(sizeof(T)), S, EF, I == 0 ? 0 : kJointWide, {I < 3, I < 2, true});
    if (c.form == k.form && c.eval == k.eval) return fn(PipeTag<k.form.joint ? k.form.s0 : 0, k.form.lag1, k.eval>{});
    with_pipe_form<T, S, EF, I + 1>(c, fn);
  } else {
    MXS_CHECK(false, "no pipeline kernel for S = " << S << ": " << c.form.s0 << " + " << c.form.s1 << ", joint "
                                                   << c.form.joint << ", lag1 " << c.form.lag1 << ", form "
                                                   << int(c.eval));
  }
}

// BP: with the in-block progress priority (pipe_block_prio_form forms only).
template <typename T, int S, bool WRAP, EvalForm EF, int JS0, int LAG1, bool BP = false>
constexpr auto pipe_kernel() {
  constexpr PipeForm P = kPerStrip<T, S, EF>;
  static_assert(!BP || pipe_block_prio_form<T, JS0, S - JS0, (JS0 > 0), LAG1, eval_sum(EF)>(),
                "no block-priority kernel in this form");
  if constexpr (JS0 > 0)
    return stencil5_stream_pipe_kernel<JS0, S - JS0, P.pf, WRAP, 0, T, eval_sum(EF), kWavesPerBlock, false, true, LAG1,
                                       eval_xb(EF), BP ? kPipeBlockPrio : 0u>;
  else
    return stencil5_stream_pipe_kernel<P.s0, P.s1, P.pf, WRAP, 0, T, eval_sum(EF)>;
}

// Fill-aware shares (balanced_starts), memoised per shape: the binary search
// costs ~10 us of host time, a launch must not.
void pipe_starts(index_t groups, index_t rows, int blocks, index_t fill, PipeShares* out, index_t last_rows = 0);

// MXS_PIPE_BALANCED=0: equal row shares (the round-2 rule), for comparison.
bool pipe_balanced();

// The shares of one pipeline pass in form `ch` over cols x rows on `blocks`
// workgroups, for the uniform and the level-table launchers alike. may_split:
// whether the kernel about to be launched can split its narrow last group
// (pipe_split_form).
template <typename T>
PipeShares pipe_pass_shares(const char* who, const TileGeom& g, const PipeChoice& ch, index_t cols, index_t rows,
                            int blocks, bool may_split) {
  const index_t groups = pipe_groups(ch.form, cols);
  // The same lengths in the share, the fill-aware starts and the kernel's own
  // `total`: the narrow last group counts split_half rows when it is split.
  const index_t split_half = pipe_split_half(ch, cols, rows);
  MXS_CHECK(split_half == 0 || may_split, who << ": this pipeline form does not split its last group");
  const index_t total = split_half > 0 ? (groups - 1) * rows + split_half : groups * rows;
  PipeShares shares = PipeShares::equal((total + blocks - 1) / blocks);  // rows per workgroup of the linear space
  shares.split_half = split_half;
  if (pipe_balanced() && blocks <= kMaxShareBlocks)
    pipe_starts(groups, rows, blocks, pipe_fill_rows(ch.form), &shares, split_half);
  // Shares longer than kMaxChunkBytes are walked in pieces inside the kernel;
  // a piece must still hold a useful number of rows.
  MXS_CHECK(chunk_rows_fit(g.pitch, sizeof(T)),
            who << ": rows of " << g.pitch * index_t(sizeof(T)) << " bytes leave fewer than " << kMinChunkRows
                << " rows per pipeline chunk (buffer-descriptor stores)");
  return shares;
}

template <typename T, int S, bool WRAP, EvalForm EF, int JS0, int LAG1>
void launch_pipe_form(const T* in, T* out, const TileGeom& g, index_t x0, index_t x1, index_t y0, index_t y1, T c0,
                      T c1, const PipeChoice& ch, hipStream_t s) {
  static_assert(EF != EvalForm::Scaled || JS0 > 0, "the scaled form runs the joint pipeline");
  static_assert(JS0 > 0 || pipe_owg(kPerStrip<T, S, EF>) == kWavesPerBlock * StripShape<T, S, true>::OW,
                "pipe_form.hpp's per-strip group is the kernel's");
  // One 512-thread workgroup per CU: the occupancy API decides, asked about
  // the descending-order sum / per-step kernel of the same windows.
  const int blocks = resident_workgroups(
      reinterpret_cast<const void*>(
          pipe_kernel<T, S, WRAP, eval_sum(EF) ? EvalForm::Sum : EvalForm::PerStep, JS0, 0>()),
      2 * kBlock, 1);
  const PipeShares shares =
      pipe_pass_shares<T>("stencil5_tb", g, ch, x1 - x0, y1 - y0, blocks,
                          pipe_split_form<T, JS0, S - JS0, kWavesPerBlock, (JS0 > 0), LAG1>());
  const KernelCoeffs<T> k = kernel_coeffs(EF, c0, c1, S);
  constexpr bool kBlockPrio = pipe_block_prio_form<T, JS0, S - JS0, (JS0 > 0), LAG1, eval_sum(EF)>();
  MXS_CHECK(!ch.block_prio || kBlockPrio, "stencil5_tb: this pipeline form has no block-priority kernel");
  auto launch = [&](auto kernel) {
    kernel<<<blocks, 2 * kBlock, 0, s>>>(in, out, g.pitch, g.core_offset(), g.width, g.height, x0, x1, y0, y1, shares,
                                         k.a, k.b);
  };
  if constexpr (kBlockPrio) {
    if (ch.block_prio) launch(pipe_kernel<T, S, WRAP, EF, JS0, LAG1, true>());
    else launch(pipe_kernel<T, S, WRAP, EF, JS0, LAG1>());
  } else {
    launch(pipe_kernel<T, S, WRAP, EF, JS0, LAG1>());
  }
  note_launch(EF == EvalForm::Scaled ? "stream_pipe_scaled" : EF == EvalForm::Sum ? "stream_pipe_sum" : "stream_pipe",
              ch.form, shares.split_half > 0, ch.block_prio);
}

template <typename T, int S, bool WRAP, EvalForm EF>
void launch_pipe_impl(const T* in, T* out, const TileGeom& g, index_t x0, index_t x1, index_t y0, index_t y1, T c0, T c1,
                      hipStream_t s) {
  const PipeChoice ch = pipe_form_for(int(sizeof(T)), S, EF, x1 - x0, pipe_switches());
  with_pipe_form<T, S, EF>(ch, [&](auto tag) {
    using K = decltype(tag);
    launch_pipe_form<T, S, WRAP, K::EF, K::JS0, K::LAG1>(in, out, g, x0, x1, y0, y1, c0, c1, ch, s);
  });
}

// Whether the fp64 wide-lane pipeline can take [x0, x1) at depth S: whole
// 4-cell lane vectors (x0, x1 and, wrapping, the width multiples of 4), the
// apron inside the row padding, and rows narrow enough for kMinChunkRows per
// descriptor-sized piece (longer chunks go in pieces).
template <typename T, int S, bool WRAP>
bool wide_pipe_ok_impl(const TileGeom& g, index_t x0, index_t x1) {
  constexpr int SA = StripShape<T, S, true>::SA;
  if (x0 % 4 != 0 || x1 % 4 != 0) return false;
  if (WRAP && g.width % 4 != 0) return false;
  const index_t lead = g.x_origin + g.halo_x;
  if (!WRAP && (lead < SA || g.pitch < lead + (g.width + 3) / 4 * 4 + SA)) return false;
  return chunk_rows_fit(g.pitch, sizeof(T));
}

// Explicitly instantiated in the pipeline TUs (the scaled form at the solver's
// depths only: fp32 20 / 24, fp64 16).
template <typename T, int S, bool WRAP, EvalForm EF>
void launch_pipe(const T* in, T* out, const TileGeom& g, index_t x0, index_t x1, index_t y0, index_t y1, T c0, T c1,
                 hipStream_t s);
template <typename T, int S, bool WRAP>
bool wide_pipe_ok(const TileGeom& g, index_t x0, index_t x1);

}  // namespace detail
}  // namespace kernels
}  // namespace mxs
