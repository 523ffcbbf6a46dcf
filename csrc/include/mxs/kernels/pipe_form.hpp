// The form of a two-stage pipeline pass (stencil_pipe_kernels.hpp:
// stencil5_stream_pipe_kernel / stencil5_pipe_chunks_kernel), chosen once for
// the one-launch and the chunk-list pass: the evaluation form, the stage split,
// the window layout and the level order, and the shape numbers that follow
// from them. Host-only (no HIP): the launchers (stencil_pipe.hpp), the policy
// (kernels.hpp: auto_time_block) and the unit tests read the same functions.
#pragma once

#include "mxs/core/config.hpp"

namespace mxs {
namespace kernels {

// How a pass evaluates its S levels: per step (c0, c1 at every level, bitwise
// equal to S single steps), or one of the fast forms, the sum form (c0 == c1)
// and the scaled form (c0 != c1, c1 != 0); see Stencil5Coeffs in kernels.hpp.
// Derived once per pass (kernels.hpp: eval_form); the only encoding above the
// kernel template arguments.
enum class EvalForm : int { PerStep = 0, Sum = 1, Scaled = 2 };
// The device templates' <SUM, XB> (stencil_bodies.hpp: FastBody).
constexpr bool eval_sum(EvalForm f) { return f != EvalForm::PerStep; }
constexpr int eval_xb(EvalForm f) { return f == EvalForm::Scaled ? 2 : 0; }
// Depths at which the scaled form has kernels: the fp32 balanced stream kernel
// (2-16) and pipeline (20 / 24), the fp64 wide pipeline (16). Elsewhere a
// scaled request runs per step.
constexpr bool scaled_depth(int elem_bytes, int S) {
  return elem_bytes == 4 ? (S > 1 && (S <= 16 || S == 20 || S == 24)) : S == 16;
}

constexpr int kPipeStrips = 4;  // column strips (stage-0 / stage-1 wave pairs) per pipeline workgroup
constexpr int kLagBoth = 3;     // level-order mask: both stages ascend

// s0 + s1 levels in the two stages, pf input rows in flight; joint: stage 1's
// windows are cut from one joint row per group (JointShape), else every strip
// carries the apron of all S levels; lag1: level-order mask (stencil_pipe_kernels.hpp
// pipe_chunk), 0 = both stages descend, kLagBoth = both ascend.
struct PipeForm {
  int s0 = 0, s1 = 0, pf = 0;
  bool joint = false;
  int lag1 = 0;
};
constexpr bool operator==(const PipeForm& a, const PipeForm& b) {
  return a.s0 == b.s0 && a.s1 == b.s1 && a.pf == b.pf && a.joint == b.joint && a.lag1 == b.lag1;
}
// The experiment switches (kernels.hpp: set_pipe_joint / _lag1 / _split /
// _block_prio), all on by default.
struct PipeSwitches {
  bool joint = true, lag1 = true, split = true, block_prio = true;
};
// A pass's form, the evaluation form it runs (a request the form has no kernel
// for falls back to per step), whether a narrow last group is split and whether
// its waves set their priority from their progress inside each block of rows.
struct PipeChoice {
  PipeForm form;
  EvalForm eval = EvalForm::PerStep;
  bool split = false;
  bool block_prio = false;
};

// With ascending levels fp32 S = 20 runs 8 + 12 below this many columns
// (8192^2: 9.49 vs 9.36 T cells/s for 12 + 8), else 12 + 8.
constexpr index_t kJointWide = 12288;

// fp32 (S = 17..32), per-step form: the fetching stage takes one level more
// than half, S0 = S/2 + 1 (at most 16) — measured 2-3% ahead of the even split
// on 4 of 5 tile shapes (profiles/r02_deep/pipe2_*, pipe20_*); sum form: the
// even split (S = 20: 10 + 10 beats 11 + 9 by 4-5% on 32768^2, 16384 x 8192 and
// 8192^2, profiles/r02_sum). 6 input rows in flight up to S = 28 (the fetch
// ring fits beside the windows at 2 waves/SIMD), 3 above. fp64 (S = 9..16,
// wide-lane body): even split, 3 rows in flight — 6 + 6 is the fastest
// per-step fp64 form on every measured tile (8192^2 3.0 vs 2.2 T cells/s for
// the single-wave natural kernel, 16384^2 3.35 vs 2.5; odd depths lose to the
// apron rounding: profiles/r02_f64), 8 + 8 the fastest sum form (3.5 / 4.05).
//
// Joint stage-1 windows (JointShape): time blocks that split into two multiples
// of 4 levels, so the joint read reach A0 + A1 equals the per-strip apron SA(S)
// and the ghost-ring / padding requirements do not change: fp32 S = 20 .. 32 in
// steps of 4, fp64 S = 16. Splits (tuner, sum form, profiles/r02_joint): 20 =
// 12 + 8 (32768^2 10.9 vs 10.7 T cells/s for 8 + 12 and 10.0 per-strip
// 10 + 10) or, ascending on tiles below kJointWide columns, 8 + 12 (2-3% ahead
// on the 16384- and 8192-wide tiles); 24 = 12 + 12 (11.1 vs 10.2 per-strip);
// 28 = 12 + 16 (11.5); 32 = 16 + 16 (11.8; PF = 3); fp64 16 = 8 + 8 (944 vs 896
// columns per group). The scaled form runs in the joint windows only: with them
// off (MXS_PIPE_JOINT=0) the pass runs per step, exact.
//
// Level order: ascending levels lag one row per level instead of three, so a
// chunk fills its pipeline S - 1 rows sooner per stage, at the cost of a
// dependent chain of levels per row. Round 2 (wall-clock tuner,
// profiles/r02_lag1) found it paying on short chunks only and kept the
// descending order past 768-row shares. Round 6 measured it in shader cycles
// per workgroup (tuner focus fillfit, profiles/r06_fill): the two orders cost
// the same per row (796 cycles per group-row at S = 20, 12 + 8) and the
// ascending one less per share (38 k vs 51 k cycles of fill), so fp32 S = 20
// ascends at every share length: 32768^2 -0.65%, 16384^2 -1.8%, the 8-GPU tile
// -2.3% workgroup cycles. S = 24 (12 + 12) took it everywhere already. fp64
// S = 16 (8 + 8): 8192^2 (288-row chunks) 3.88 -> 4.00 T cells/s
// (profiles/r02_lag1/*64*); on 2240-row shares (32768 x 16384) the two orders
// tie (4,354 vs 4,346 G cells/s, profiles/r06_fp64), so fp64 ascends at every
// share length too. The other joint depths descend.
//
// The narrow last group splits (stencil_pipe_kernels.hpp: pipe_split_form) in the
// fp32 12 + 12 ascending form only.
//
// In-block progress priority (stencil_pipe_kernels.hpp: pipe_chunk BPRIO,
// pipe_block_prio_form): the fp32 joint forms in ascending order, S = 20 and
// 24, in the sum and scaled forms (profiles/pipe_prio). The per-step bodies
// keep equal priorities: s_setprio fences the instruction scheduler, and with
// it they grow from 207-217 to 244-256 VGPRs. So do fp64 8 + 8 (HBM-bound) and
// the descending forms.
constexpr PipeChoice pipe_form_for(int elem_bytes, int S, EvalForm eval, index_t columns, PipeSwitches on = {}) {
  const bool f32 = elem_bytes == 4;
  PipeChoice c;
  c.eval = (eval == EvalForm::Scaled && !scaled_depth(elem_bytes, S)) ? EvalForm::PerStep : eval;
  c.form.pf = (f32 && S <= 28) ? 6 : 3;
  c.form.joint = on.joint && (f32 ? (S % 4 == 0 && S >= 20) : S == 16);
  if (c.form.joint) {
    const bool ascend = on.lag1 && (f32 ? (S == 20 || S == 24) : S == 16);
    c.form.lag1 = ascend ? kLagBoth : 0;
    c.form.s0 = !f32 ? S / 2 : S >= 32 ? 16 : (S == 20 && ascend && columns < kJointWide) ? 8 : 12;
    c.split = on.split && f32 && c.form.s0 == 12 && S == 24 && ascend;
    c.block_prio = on.block_prio && f32 && ascend && c.eval != EvalForm::PerStep;
  } else {
    if (c.eval == EvalForm::Scaled) c.eval = EvalForm::PerStep;
    c.form.s0 = (!f32 || c.eval == EvalForm::Sum) ? S / 2 : (S / 2 + 1 < 16 ? S / 2 + 1 : 16);
  }
  c.form.s1 = S - c.form.s0;
  return c;
}

namespace detail {

// Joint stage-1 windows (JOINT). In the per-strip layout every strip pays the
// apron of all S levels: 256 - 2 SA(S) output columns per strip (208 of 256 at
// S = 24). Stage 1 does not need its own strip's stage-0 edges, though: the
// level-S0 columns a stage-0 wave gets right (all but A0 = S0 rounded up to 4
// per side) are laid side by side, for the G strips of the workgroup, in ONE
// LDS row of G * OW0 valid columns, and stage 1's G windows (256 columns each,
// stride OW1 = 256 - 2 A1) are cut from that row. Stage 0's apron is still
// paid per strip, stage 1's once per group: OWG = G (256 - 2 A0) - 2 A1 output
// columns per group, capped at G * OW1 (S = 24 as 12 + 12: 904 vs 4 x 208 =
// 832, +8.7% per pass at the same VALU work; S = 20 as 8 + 12: 928 vs 864;
// S = 28 as 12 + 16: 896 vs 800). The stage-0 lanes that hold no valid
// column write into the row's tail (G * 2 A0 / 4 slots, exactly the lanes that
// need one), which stage 1 only reads into columns it never stores. Same
// operations per cell as the per-strip layout: bitwise identical output.
template <int S0, int S1, int G>
struct JointShape {
  static constexpr int A0 = (S0 + 3) / 4 * 4, A1 = (S1 + 3) / 4 * 4;  // per-stage aprons (4-column lanes)
  static constexpr int OW0 = 256 - 2 * A0;    // valid level-S0 columns per stage-0 wave
  static constexpr int OW1 = 256 - 2 * A1;    // stride of stage 1's windows
  static constexpr int SPAN = G * OW0;        // valid columns of the joint row
  // Output columns per group: the joint row's valid span less stage 1's apron,
  // or what the G windows can store (G * OW1) when that is less (A0 < A1).
  static constexpr int OWG = SPAN - 2 * A1 < G * OW1 ? SPAN - 2 * A1 : G * OW1;
  static constexpr int ROW = G * kWaveSize;   // joint row length in lane vectors (SPAN / 4 + the tail)
  static constexpr int LEAD = A0 + A1;        // input columns left of the group's first output column
  static_assert((G - 1) * OW1 + 256 <= 4 * ROW, "stage-1 windows must stay inside the joint row");
  static_assert(OWG > 0, "time block too deep for a joint group");
};

template <typename T, int S0, int S1, int G, bool JOINT, int LAG1>
constexpr bool pipe_split_form() {
  return JOINT && sizeof(T) == 4 && G == 4 && S0 == 12 && S1 == 12 && LAG1 == 3;
}
// The forms that have kernels with the in-block progress priority.
template <typename T, int S0, int S1, bool JOINT, int LAG1, bool SUM>
constexpr bool pipe_block_prio_form() {
  return JOINT && SUM && sizeof(T) == 4 && LAG1 == kLagBoth && (S0 + S1 == 20 || S0 + S1 == 24);
}

}  // namespace detail

// ------------------------------------------------------------ shape numbers
// Run-time twins of the constexpr shapes the kernels are built from (checked
// against them below and in stencil_pipe.hpp).
constexpr int apron4(int levels) { return (levels + 3) / 4 * 4; }  // 4-column lanes
// Output columns of a joint group of `strips` strips (JointShape::OWG).
constexpr int joint_owg(int s0, int s1, int strips) {
  const int span = strips * (256 - 2 * apron4(s0)), cap = strips * (256 - 2 * apron4(s1));
  return span - 2 * apron4(s1) < cap ? span - 2 * apron4(s1) : cap;
}
// Output columns per workgroup pass over a row: a joint group, or kPipeStrips
// strips of 256 - 2 SA(S) columns.
constexpr int pipe_owg(const PipeForm& f) {
  return f.joint ? joint_owg(f.s0, f.s1, kPipeStrips) : kPipeStrips * (256 - 2 * apron4(f.s0 + f.s1));
}
constexpr index_t pipe_groups(const PipeForm& f, index_t columns) { return (columns + pipe_owg(f) - 1) / pipe_owg(f); }
// Input columns a group reads left of its first output column (and right of
// its last): the joint read reach A0 + A1 (JointShape::LEAD), per strip SA(S).
constexpr int pipe_apron(const PipeForm& f) {
  return f.joint ? apron4(f.s0) + apron4(f.s1) : apron4(f.s0 + f.s1);
}
// A joint group whose first output column is x reads input columns
// [x - pipe_apron, x - pipe_apron + pipe_read_span).
constexpr int pipe_read_span(const PipeForm& f) { return (kPipeStrips - 1) * (256 - 2 * apron4(f.s0)) + 256; }
// Row iterations a chunk of R rows costs beyond R (pipe_chunk: the longer of
// the two stages' block counts, rounded up to a block).
constexpr index_t pipe_fill_rows(int s0, int s1, int pf, int lag1) {
  const int e0 = (lag1 & 1) ? 2 * s0 : 3 * s0 - 1, e1 = (lag1 & 2) ? 2 * s1 : 3 * s1 - 1;
  const int d = (pf - e0 % pf) % pf;
  const int t1 = (e0 + d) / pf + 1;
  const int a = 2 * s1 + e0 + d, b = t1 * pf + e1;
  return (a > b ? a : b) + pf - 1;
}
constexpr index_t pipe_fill_rows(const PipeForm& f) { return pipe_fill_rows(f.s0, f.s1, f.pf, f.lag1); }
// Length of the split narrow last group in the linear (group x rows) space,
// ceil(rows / 2), or 0 when the pass does not split: another form, the switch
// off, or more columns left for the last group than a two-strip joint group
// stores (440 at 12 + 12).
constexpr index_t pipe_split_half(const PipeChoice& c, index_t columns, index_t rows) {
  if (!c.split) return 0;
  const index_t rem = columns - (pipe_groups(c.form, columns) - 1) * pipe_owg(c.form);
  return rem <= joint_owg(c.form.s0, c.form.s1, kPipeStrips / 2) ? (rows + 1) / 2 : 0;
}

namespace detail {
template <int S0, int S1, int LAG1 = 0>
constexpr bool joint_twin_ok() {
  using J = JointShape<S0, S1, kPipeStrips>;
  constexpr PipeForm f{S0, S1, 6, true, LAG1};
  return pipe_owg(f) == J::OWG && pipe_apron(f) == J::LEAD && pipe_read_span(f) == (kPipeStrips - 1) * J::OW0 + 256 &&
         joint_owg(S0, S1, kPipeStrips / 2) == JointShape<S0, S1, kPipeStrips / 2>::OWG &&
         pipe_form_for(4, S0 + S1, EvalForm::Sum, 0, {true, LAG1 != 0, true}).split ==
             pipe_split_form<float, S0, S1, kPipeStrips, true, LAG1>() &&
         pipe_form_for(4, S0 + S1, EvalForm::Sum, 0, {true, LAG1 != 0}).block_prio ==
             pipe_block_prio_form<float, S0, S1, true, LAG1, true>() &&
         !pipe_form_for(4, S0 + S1, EvalForm::PerStep, 0, {true, LAG1 != 0}).block_prio;
}
static_assert(joint_twin_ok<8, 12, kLagBoth>() && joint_twin_ok<12, 8, kLagBoth>() && joint_twin_ok<12, 8>() &&
                  joint_twin_ok<12, 12, kLagBoth>() && joint_twin_ok<12, 12>() && joint_twin_ok<12, 16>() &&
                  joint_twin_ok<16, 16>() && joint_twin_ok<8, 8>(),
              "the run-time shape numbers follow JointShape / pipe_split_form / pipe_block_prio_form");
}  // namespace detail

// Output columns per group of the two forms auto_time_block weighs (the
// default fp32 forms on wide tiles).
constexpr int kOwgS20 = 912, kOwgS24 = 904;
static_assert(kOwgS20 == detail::JointShape<12, 8, kPipeStrips>::OWG && kOwgS24 == detail::JointShape<12, 12, kPipeStrips>::OWG,
              "auto_time_block counts the groups of the 12 + 8 and 12 + 12 joint forms");

}  // namespace kernels
}  // namespace mxs
