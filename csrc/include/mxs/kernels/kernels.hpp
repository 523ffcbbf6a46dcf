// Host API of the hand-written CDNA4 (gfx950) kernels. Every launcher is
// stream-ordered, allocation-free and synchronisation-free, so any sequence of
// them can be captured into a hipGraph (cdna_hip_programming.md Guideline 9).
//
// Kernel inventory:
//   K1/K3  fill, fill_region, fill_random       kernels/fill.hip
//   K10    stencil5_rows / stencil5_rect         kernels/stencil.hip
//          stencil_box (LDS-tiled (2R+1)^2)      kernels/stencil.hip
//   K11/12 copy2d_batch (halo pack/unpack/self)  kernels/halo.hip
//   K2/4/5/8 dot_atomic, dot_partials, reduce_partials, dot_single_pass, dot_racy
//                                                kernels/dot.hip
//          stencil5_residual (norms of A u - u)  kernels/residual.hip
//          stencil5_tb_held (fixed-edge frame)   kernels/stencil_held.hip
//   K13    level passes (Chebyshev cycles), with or without a correction tile; source_axpy (the source term)
//                                                kernels/stencil_levels.hip, stencil_pipe_levels[_src]_f32/_f64.hip
//          mg_smooth, mg_residual_restrict, mg_prolong_add, mg_coarse_solve (the multigrid V-cycle)
//                                                kernels/multigrid.hip
//          cg_start, cg_apply, cg_update (conjugate gradients with fused dot products)
//          pcg_start, pcg_apply, pcg_update (the same bodies for preconditioned CG) kernels/cg.hip
//          cg_heat_start, pcg_heat_start (the start of an implicit heat step: right-hand side and residual in one pass)
//          mgp_smooth, mgp_residual_restrict, mgp_prolong_add, mgp_coarse_solve (the any-size
//          V-cycle preconditioner: the same kernels with ghost codes)  kernels/multigrid.hip
//                                                kernels/cg.hip
#pragma once

#include <hip/hip_runtime_api.h>

#include <cmath>
#include <cstdint>
#include <limits>

#include "mxs/grid/layout.hpp"
#include "mxs/kernels/cg.hpp"
#include "mxs/kernels/chunk_schedule.hpp"
#include "mxs/kernels/fixed_edge_split.hpp"
#include "mxs/kernels/heat.hpp"
#include "mxs/kernels/multigrid.hpp"
#include "mxs/kernels/pcg.hpp"
#include "mxs/kernels/pipe_form.hpp"
#include "mxs/kernels/relaxation.hpp"

namespace mxs {
namespace kernels {

// ---------------------------------------------------------------- fill (K1/K3)
template <typename T>
void fill(T* p, index_t n, T value, hipStream_t s);
// Fill a window of a buffer (reference InitKernel, stencil2d/mpi-2d-stencil-subarray-cuda.cu:17-28,
// which launched one thread per block).
template <typename T>
void fill_region(T* base, const Array2D& region, T value, hipStream_t s);
// Deterministic pseudo-random init of the core of a tile in [lo, hi): the value of
// a cell depends only on its *global* coordinates and the seed, so any domain
// decomposition of the same global grid starts from bit-identical data.
template <typename T>
void fill_random(T* tile, const TileGeom& g, index_t global_x0, index_t global_y0,
                 index_t global_width, std::uint64_t seed, T lo, T hi, hipStream_t s);

// ------------------------------------------------------------- stencil (K10)
// out = c_center * u[y][x] + c_neighbor * ((u[y-1][x] + u[y+1][x]) + (u[y][x-1] + u[y][x+1]))
// evaluated as fma(c_neighbor, (n + s) + (w + e), c_center * c) in the element type, so
// every kernel variant and the host reference agree bit for bit.
struct Stencil5Coeffs {
  double center = 0.2;
  double neighbor = 0.2;
  // With center == neighbor (= c, the 5-point average) the S-step kernels may
  // run the sum form: each pass accumulates plain 5-point sums and scales by
  // c^S once when it stores (8 instead of 11 VALU issue slots per 4 fp32 cells
  // and step; stencil_bodies.hpp). Equal to the per-step evaluation up to
  // rounding (a few ulp), not bit for bit. With center != neighbor (neighbor
  // != 0) the pipeline passes run the scaled form instead: v' = (n + s + w + e)
  // + (center / neighbor) v per level, neighbor^S once per pass (9 instead of 11
  // slots). false = always the per-step form.
  bool sum_form = true;
  // Bound on max|u| of a pass's input field (the solver passes its measured,
  // agreed absmax), or < 0: unknown. See fast_form_safe().
  double range = -1.0;
};
// The fast form the coefficients ask for, before any bound (eval_form): the sum
// form (equal coefficients) or the scaled form (unequal, c_neighbor != 0; it has
// kernels in the fp32 pipeline (20 / 24) and balanced stream kernel (2-16) and
// the fp64 wide pipeline (16); other depths and kernel forms run per step).
inline EvalForm requested_form(const Stencil5Coeffs& c) {
  if (!c.sum_form || c.neighbor == 0.0) return EvalForm::PerStep;
  return c.center == c.neighbor ? EvalForm::Sum : EvalForm::Scaled;
}
// The guard of both fast forms for an S-level pass in element type T, stated
// once: stencil5_tb and the chunk pass choose their form through it, and the
// solver calls it with its measured, agreed range:
//   * |c_center| + 4 |c_neighbor| <= 1: the operator is bounded by the field;
//   * c_neighbor^S is a normal number of T (it scales the stored result);
//   * inside a pass the carried values grow by up to (4 + |k|)^S (k =
//     c_center / c_neighbor; 5^S for the sum form): range (4 + |k|)^S < max/4.
// With the range unknown (range < 0) only a form that grows no faster than the
// sum form (|k| <= 1) is taken, under the sum form's documented contract
// (max|u| 5^S < max/4 is the caller's); a faster-growing scaled form runs per
// step (c_center 0.9, c_neighbor 0.013 grows as 73^S: 2e37 at S = 20).
enum class FastFormVerdict : int {
  Ok = 0,
  NotFastPair,      // sum_form off, or c_neighbor == 0
  Unbounded,        // |c_center| + 4 |c_neighbor| > 1
  ScaleSubnormal,   // c_neighbor^S below the normal range of T
  RangeOverflow,    // range (4 + |k|)^S >= max/4 (or the range is not finite)
  RangeUnknownGrowth,  // range unknown and |k| > 1
};
template <typename T>
inline FastFormVerdict fast_form_verdict(const Stencil5Coeffs& c, int S) {
  if (requested_form(c) == EvalForm::PerStep) return FastFormVerdict::NotFastPair;
  if (!(std::fabs(c.center) + 4.0 * std::fabs(c.neighbor) <= 1.0 + 1e-6)) return FastFormVerdict::Unbounded;
  if (!(std::fabs(double(T(std::pow(c.neighbor, double(S))))) >= double(std::numeric_limits<T>::min())))
    return FastFormVerdict::ScaleSubnormal;
  const double k = std::fabs(c.center / c.neighbor);
  if (c.range < 0.0) return k <= 1.0 ? FastFormVerdict::Ok : FastFormVerdict::RangeUnknownGrowth;
  const bool fits =
      std::isfinite(c.range) && c.range * std::pow(4.0 + k, double(S)) < double(std::numeric_limits<T>::max()) / 4.0;
  return fits ? FastFormVerdict::Ok : FastFormVerdict::RangeOverflow;
}
template <typename T>
inline bool fast_form_safe(const Stencil5Coeffs& c, int S) {
  return fast_form_verdict<T>(c, S) == FastFormVerdict::Ok;
}
// The evaluation form of an S-level pass: the requested fast form inside its
// bounds, else per step.
template <typename T>
inline EvalForm eval_form(const Stencil5Coeffs& c, int S) {
  return fast_form_safe<T>(c, S) ? requested_form(c) : EvalForm::PerStep;
}

enum class StencilVariant : int {
  Auto = 0,        // tuned default
  RegisterRoll = 1,  // rolling 3-row register window, x-neighbours by wave shuffles
  LdsTile = 2,       // LDS-staged 2D tile with a 1-cell ring
};

// Update core rows [row_begin, row_end) over the full core width. Columns 0 and
// width-1 read the ghost columns, so the result is only final once the halo for
// the current iteration has landed (see StencilSolver for the overlap schedule).
template <typename T>
void stencil5_rows(const T* in, T* out, const TileGeom& g, index_t row_begin, index_t row_end,
                   Stencil5Coeffs c, hipStream_t s, StencilVariant v = StencilVariant::Auto);

// Full-tile update of a 1x1 periodic grid with the self-exchange fused into the
// addressing (row -1 reads row H-1, column W reads column 0, ...): one launch per
// iteration, no ghost traffic. Needs width % (16 / sizeof(T)) == 0.
template <typename T>
void stencil5_periodic(const T* in, T* out, const TileGeom& g, Stencil5Coeffs c, hipStream_t s);
template <typename T>
bool stencil5_periodic_supported(const TileGeom& g);

// Temporal blocking: `steps` (S) Jacobi iterations in one launch over the core
// rectangle [x0, x1) x [y0, y1): every input byte crosses HBM once per S
// iterations. The source must hold valid data S cells around the rectangle: a
// ghost ring >= S deep exchanged for this super-step, or `wrap` (1x1 periodic
// grid: reads wrap around the tile). Bitwise identical to S single steps (same
// per-cell fma sequence). Variants:
//   Auto         wave-streaming kernel (register windows per time level, no LDS)
//                for the bulk, LDS tiles of matching shape for thin strips;
//   LdsTile      LDS-tiled (each workgroup stages its tile plus an S-deep apron,
//                iterates in LDS; S <= 8 for the bulk tile);
//   RegisterRoll same as Auto.
constexpr int kMaxTimeBlock = 16;
// fp32 blocks of 17..32 steps run on the two-stage wave pipeline
// (stencil5_stream_pipe_kernel: two waves per column strip, levels split
// between them and handed over through LDS). Needs fp32, x0 and x1 multiples
// of 4 (whole vectors); see stencil5_deep_supported().
constexpr int kMaxTimeBlockDeep = 32;
// Largest chunk (rows x pitch bytes) one workgroup of the streaming kernels
// stores through a single buffer descriptor: below 2^31 with room for the
// drop offsets of stencil_stream.hpp and stencil_pipe_kernels.hpp (a sum of two never wraps).
constexpr index_t kMaxChunkBytes = 0x7F000000;
// The wave pipelines walk a longer share in pieces of at most kMaxChunkBytes;
// rows must be narrow enough that a piece holds at least this many (each piece
// pays its own pipeline fill of S rows).
constexpr index_t kMinChunkRows = 64;
// Whether `rows` rows of `pitch` elements fit one descriptor-sized piece.
constexpr bool chunk_rows_fit(index_t pitch, int elem_bytes, index_t rows = kMinChunkRows) {
  return pitch * elem_bytes * rows <= kMaxChunkBytes;
}
// Measured default S for a w x h tile of `elem_bytes`-byte cells
// (profiles/stencil_tuning/tunes_*, profiles/r02_deep/pipe*_*, profiles/r02_f64,
// profiles/r02_sum): fp32 takes the two-stage pipeline at S = 20 (sum form,
// split 10 + 10: 32768^2 9.96 T cells/s, 16384 x 8192 9.18, 8192^2 7.79; the
// per-step form 11 + 9: 8.27 / 7.56 / 6.46; S = 24-28 adds 2-4% at 32768^2
// only); fp64 the wide-lane pipeline at S = 16 in the sum form (8 + 8: 3.5 /
// 4.05 T cells/s at 8192^2 / 16384^2) or S = 12 per step (6 + 6: 3.0 / 3.3);
// the fp32 single-wave kernels (small tiles): S = 16 from 2^27 cells, S = 12
// below (the pass is VALU-bound beyond S ~ 8, so a deeper block only pays
// where the chunk / strip aprons are small against the tile).
inline int auto_time_block(index_t w, index_t h, int elem_bytes = 4, bool sum_form = true) {
  // Rows too wide for kMinChunkRows per descriptor-sized piece (beyond ~8.3 M
  // fp32 columns; the padded pitch is at most w + 256): the fp32 pipelines
  // cannot take them, the single-wave kernels can (their non-descriptor body).
  if (elem_bytes == 4 && !chunk_rows_fit(w + 256, 4)) return kMaxTimeBlock;
  if (elem_bytes == 4 && w >= 1024 && h >= 1024) {
    // The pipeline runs workgroups of 4 strips; with joint stage-1 windows a
    // group stores kOwgS20 = 912 columns at S = 20 (12 + 8) and kOwgS24 = 904
    // at S = 24 (12 + 12).
    // A partial last group costs a whole one, except at S = 24 (ascending
    // order) when at most 440 columns are left for it: then it is split and
    // costs half (set_pipe_split). S = 24 when it needs no more groups than
    // S = 20 (4096 wide: 5 and 5); otherwise the extra group cost more than
    // the deeper block saved when this rule was measured, with whole last
    // groups (8192^2 sum form: 9 vs 10 groups, 8.6-8.9 T cells/s at S = 20 vs
    // 8.4 at 24; 16384 wide: 18 vs 19 groups, 9.8-10.0 vs 9.4;
    // profiles/r02_joint). With the split (9.5 and 18.5 groups) S = 24 measures
    // 1.3% (8192^2) and 3.8% (16384 x 8192) ahead of S = 20 in paired 240-step
    // windows (profiles/pipe_split); the rule is kept as it is pinned by the
    // policy test, the 8192^2 rate floor and the config-2 cycle budget.
    auto groups = [&](int owg) { return (w + owg - 1) / owg; };
    if (sum_form && groups(kOwgS24) <= groups(kOwgS20)) return 24;
    // Tiles of >= 2^30 cells (chunks of ~4800 rows, warm-up negligible): the
    // deeper block relieves HBM and wins even at one group more, 32768^2 sum
    // form 11.1 T cells/s at S = 24 vs 10.9 at 20 (37 vs 36 groups). A 20-step
    // run is still one S = 20 pass (run(K) splits K near-equally).
    if (sum_form && w * h >= (index_t(1) << 30)) return 24;
    return 20;
  }
  if (elem_bytes == 8) return sum_form ? 16 : 12;
  return w * h >= (index_t(1) << 27) ? 16 : 12;
}
// Whether a `steps`-step stencil5_tb launch over [x0, x1) can run: every
// steps <= kMaxTimeBlock; deeper blocks only for fp32 on whole vectors.
template <typename T>
constexpr bool stencil5_deep_supported(int steps, index_t x0, index_t x1) {
  return steps <= kMaxTimeBlock || (steps <= kMaxTimeBlockDeep && sizeof(T) == 4 && x0 % 4 == 0 && x1 % 4 == 0);
}
template <typename T>
void stencil5_tb(const T* in, T* out, const TileGeom& g, int steps, index_t x0, index_t x1, index_t y0, index_t y1,
                 Stencil5Coeffs c, bool wrap, hipStream_t s, StencilVariant v = StencilVariant::Auto);

// The same contract as stencil5_tb(..., wrap = false) over [x0, x1) x [y0, y1),
// except that at every one of the `steps` levels a cell outside the core on a
// held side (`hold`: HoldSide bits, fixed_edge_split.hpp) keeps its input value:
// the fixed boundary values of a physical edge. Ghost cells on the other sides
// advance as cells (they are a neighbour's). An LDS tile that recomputes its
// whole staged window at every level in the per-step form only: bitwise equal to
// `steps` single steps, and with hold == 0 to the per-step stencil5_tb. Tile
// shapes follow the rectangle (tall narrow for column strips, wide flat for row
// strips, one general tile): it is meant for the frame of fixed_edge_split(),
// not for the bulk. fp32 steps 1..kMaxTimeBlockDeep, fp64 1..kMaxTimeBlock.
template <typename T>
void stencil5_tb_held(const T* in, T* out, const TileGeom& g, int steps, index_t x0, index_t x1, index_t y0, index_t y1,
                      Stencil5Coeffs c, unsigned hold, hipStream_t s);

// --------------------------------- level-table passes (Chebyshev relaxation)
// One pass of t.n levels where level l runs fma(neighbor[l], (n + s) + (w + e),
// center[l] * c): a Chebyshev cycle (relaxation.hpp). The table's doubles are
// rounded to T once on the host and travel in the kernel arguments, so a
// captured launch replays the same table. Depths: relaxation_depth_supported().
// stencil5_tb_levels keeps the contract of stencil5_tb(..., wrap = false) in the
// per-step form: the two-stage pipeline in the form pipe_form_for() picks for
// the uniform per-step pass ("stream_pipe_levels"), or, for a rectangle the
// pipeline cannot take (no whole 4-cell vectors, thin strips), the held tile
// with no side held. stencil5_tb_held_levels keeps the contract of
// stencil5_tb_held ("held_levels"). Both are bitwise equal to t.n single steps
// with the levels' coefficients.
// `corr` is nullptr, or a correction tile of geometry g (the source term,
// docs/ARCHITECTURE.md "Source term"): the pass then ends with out += corr on
// the rectangle, one rounded add per cell, inside the same launch
// ("stream_pipe_levels_src" / "held_levels_src"): bitwise the pass without corr
// followed by that add. Only the rectangle's cells of corr are read, so its
// ghost ring and padding may hold anything. Kernels: stencil_levels.hip,
// stencil_pipe_levels[_src]_f32/_f64.hip.
static_assert(kMaxLevels == kMaxTimeBlockDeep, "a level table holds the deepest time block");
template <typename T>
void stencil5_tb_levels(const T* in, T* out, const TileGeom& g, index_t x0, index_t x1, index_t y0, index_t y1,
                        const LevelTable& t, const T* corr, hipStream_t s);
template <typename T>
void stencil5_tb_held_levels(const T* in, T* out, const TileGeom& g, index_t x0, index_t x1, index_t y0, index_t y1,
                             const LevelTable& t, unsigned hold, const T* corr, hipStream_t s);
// The build step of the correction: tile core += T(w) * src core with fixed
// rounding points (the product rounded, then the sum; never an fma), so it
// equals a rounded multiply and a rounded add of any other implementation.
template <typename T>
void source_axpy(T* tile, const T* src, const TileGeom& g, double w, hipStream_t s);

// ------------------------------------- chunk-list pass (interior-first super-step)
// The S-step pass over chunks of the core of a ghost-ring tile (no wrap) on the
// two-stage pipeline: workgroup w runs the chunk list table[w * entries ..]
// (kernels/chunk_schedule.hpp). Bitwise identical, per cell, to stencil5_tb
// over the same core (same per-cell arithmetic and kernel body; only the
// workgroup-to-chunk assignment differs).
struct ChunkPassShape {
  int steps = 0;
  PipeForm form;      // joint windows: stage split and level order (pipe_form.hpp)
  EvalForm eval = EvalForm::PerStep;
  int blocks = 0;     // resident workgroups (one per CU)
  index_t groups = 0;  // column groups of OWG output columns over the core width
  index_t owg = 0;
  index_t fill = 0;    // pipeline-fill row iterations per chunk
  // Input columns a group's joint windows read: [x - read_lead, x - read_lead +
  // read_span) for a group whose first output column is x (its chunks read the
  // ghost columns when that range leaves [0, width)).
  index_t read_lead = 0, read_span = 0;
};
// False when `steps` has no chunk-list form here (fp32 S = 20 / 24, fp64
// S = 16 on whole lane vectors; other depths keep the one-launch pass). The
// caller still has to keep every chunk of its schedule within kMaxChunkBytes
// (rows x pitch: the kernel's buffer-descriptor stores).
template <typename T>
bool chunk_pass_shape(const TileGeom& g, int steps, const Stencil5Coeffs& c, ChunkPassShape* out);
// table: shape.blocks x entries chunks in device memory (ChunkSchedule::table).
template <typename T>
void stencil5_chunk_pass(const T* in, T* out, const TileGeom& g, const Stencil5Coeffs& c, const ChunkPassShape& shape,
                         const PassChunk* table, int entries, hipStream_t s);

// max |x[i]| over n elements into *out (device pointer, overwritten; NaN if
// any element is NaN): the range check of the sum form.
template <typename T>
void absmax(const T* x, index_t n, T* out, hipStream_t s);
// ------------------------------------------------- residual norms (kernels/residual.hip)
// For the Jacobi update u' = A u the residual r = A u - u is exactly the change
// the next single step would make. Over the core of a ghost-ring tile, per cell
//   r = fma(c_neighbor, (n + s) + (w + e), c_center * v) - v
// in the element type (the stencil kernels' expression and order, then one
// subtraction), reduced to linf = max |r| (NaN if any r is NaN) and sumsq =
// sum r^2 accumulated in double. Reads only the core and the ring cells beside
// it (row -1, row height, column -1, column width): deeper ring layers, the
// four outside corners and the alignment padding never influence the result.
// One streaming read, no write to the tile. Deterministic: the same input gives
// the same bits in both outputs on every call (per-workgroup partials, a
// last-block finish in a fixed order; the grid depends only on the geometry and
// the CU count). sum_form / range of the coefficients are ignored.
struct ResidualNorms {  // device layout: what the kernel leaves in *out
  double linf;
  double sumsq;
};
// Workgroups of the launch at most (either element type): `partials` holds
// 2 * residual_grid_size(g) doubles, `counter` one unsigned (zeroed by the
// launcher every call, as for dot).
int residual_grid_size(const TileGeom& g);
template <typename T>
void stencil5_residual(const T* u, const TileGeom& g, Stencil5Coeffs c, ResidualNorms* out, double* partials,
                       unsigned* counter, hipStream_t s, const T* src = nullptr);
// src: a tile of geometry g whose core holds the additive term g of
// u' = A u + g; the residual is then r = (fma(...) + g) - v, each one rounded
// operation. Only core cells of src are read. Same grid, determinism and finish.

// ------------------------------------------------- multigrid (kernels/multigrid.hip)
// The four kernels of the geometric multigrid V-cycle for u = A u + g on a
// core with a depth-1 Dirichlet ring (multigrid.hpp; docs/ARCHITECTURE.md
// "Multigrid"). Every tile has a ghost ring at least 1 deep; only the cells
// named are read or written, so rings and padding of the other tiles may hold
// anything. Each is bitwise equal to its reference in ops/multigrid.py.
//
// mg_smooth: t.n (1..kMgMaxSmooth) sweeps in one launch ("mg_smooth"): reads
// u_in (core and ring) and the core of src, writes the core of u_out; ring
// cells are held. u_in != u_out. Any width, height >= 1.
template <typename T>
void mg_smooth(const T* u_in, T* u_out, const T* src, const TileGeom& g, const MgSweepTable& t, hipStream_t s);
// mg_residual_restrict: the coarse right-hand side 4 R r of the fine residual
// r = (A u + g) - u with full weighting R ("mg_residual_restrict"): reads u
// (core and ring) and the core of src once, writes the core of coarse_src. The
// coarse tile is ((width - 1) / 2) x ((height - 1) / 2), width and height odd.
template <typename T>
void mg_residual_restrict(const T* u, const T* src, const TileGeom& g, T* coarse_src, const TileGeom& gc,
                          Stencil5Coeffs c, hipStream_t s);
// mg_prolong_add: u core += P e, bilinear with e = 0 outside the coarse core
// ("mg_prolong_add"): reads the core of e, reads and writes the core of u.
template <typename T>
void mg_prolong_add(const T* e, const TileGeom& gc, T* u, const TileGeom& g, hipStream_t s);
// mg_coarse_solve: `repeats` x t.n sweeps from e = 0 on a grid of at most
// kMgCoarsestMax x kMgCoarsestMax in one workgroup's LDS ("mg_coarse_solve"):
// reads the core of src, writes the core of e.
template <typename T>
void mg_coarse_solve(const T* src, T* e, const TileGeom& g, const MgSweepTable& t, int repeats, hipStream_t s);
// The kernel the most recent multigrid launcher of this host process ran (the
// names above; "" before the first): a host-side record like
// last_stencil_dispatch(), not updated by graph replays.
const char* last_multigrid_dispatch();

// ------------------------------------------------- conjugate gradients (kernels/cg.hip)
// The three kernels of one-process CG for L u = b, L v = (1 - c0) v - c1 (n + s
// + w + e), on a core with a depth-1 Dirichlet ring (cg.hpp; docs/ARCHITECTURE.md
// "Conjugate gradients"). Tiles share one geometry with a ring at least 1 deep;
// any width, height >= 1. Each fuses its dot products: per-workgroup partials
// and a last-block finish in a fixed order (the stencil5_residual recipe), all
// sums and scalars in double, no floating-point atomics, no workgroup waits on
// another. `partials` holds 2 * cg_grid_size(g) doubles; `counter` is one
// unsigned that is 0 before the first launch (the last workgroup of every
// launch puts the 0 back). With scalars->status != 0 at entry cg_apply and
// cg_update store nothing at all. Each is bitwise equal to its reference in
// ops/cg.py; the sums differ from it by their order only.
//
// cg_start ("cg_start"): r = (fma(c1, (n + s) + (w + e), c0 v) + g) - v over
// the core, read from u with its ring and the core of g; p = r. Writes the
// cores of r and p. Last workgroup: rr, linf, beta = 0, alpha = 0, pq = 0,
// iteration = 0, status (1 if the chosen norm <= tol, else 2 if max_iters <= 0,
// else 0). tol, max_iters and norm are the host's.
int cg_grid_size(const TileGeom& g);
template <typename T>
void cg_start(const T* u, const T* g, T* r, T* p, const TileGeom& geom, Stencil5Coeffs c, CgScalars* scalars,
              double* partials, unsigned* counter, hipStream_t s, GhostSides sides = {});
// cg_apply ("cg_apply"): p_new = fma(T(beta), p_old, r); q = fma(-c1, (n + s) +
// (w + e), T(1 - c0) p_new) with p_new = 0 outside the core. The neighbours'
// p_new in a workgroup's one-cell apron are recomputed from r and p_old (same
// formula, same bits). Reads the cores of r and p_old only, writes the cores of
// p_new and q; p_old != p_new. Last workgroup: pq = sum p_new q, alpha = rr / pq
// if pq > 0 and finite, otherwise alpha = 0 and status = 3.
template <typename T>
void cg_apply(const T* r, const T* p_old, T* p_new, T* q, const TileGeom& geom, Stencil5Coeffs c, CgScalars* scalars,
              double* partials, unsigned* counter, hipStream_t s, GhostSides sides = {});
// Sides (`sides`, cg.hpp's GhostSides: ring or mirror, all ring by default):
// on a mirror side cg_start reads the ghost as edge + ring (one T addition, the
// ring cell holding the prescribed difference d) and cg_apply as the edge cell
// of p_new itself; only the global edges of the core mirror. With no mirror
// side the launchers run the ring-only kernels, bit for bit as before.
//
// cg_update ("cg_update"): u = fma(T(alpha), p, u), r = fma(-T(alpha), q, r)
// in place over the cores. Last workgroup: rr' = sum r^2, linf, beta = rr' / rr,
// rr = rr', ++iteration, status (1 if the chosen norm <= tol, else 2 if
// iteration == max_iters).
template <typename T>
void cg_update(T* u, T* r, const T* p, const T* q, const TileGeom& geom, CgScalars* scalars, double* partials,
               unsigned* counter, hipStream_t s);
// The kernel the most recent CG launcher of this host process ran ("" before
// the first); not updated by graph replays.
const char* last_cg_dispatch();

// ---------------------------- preconditioned CG (kernels/cg.hip, kernels/multigrid.hip)
// CG preconditioned by one any-size V-cycle (pcg.hpp; docs/ARCHITECTURE.md
// "Preconditioned CG"). The pcg_* kernels are the cg_* bodies on a PcgScalars
// block: the same expressions, grids, partials (2 * cg_grid_size(g) doubles) and
// ticket; with scalars->status != 0 at entry pcg_apply and pcg_update store
// nothing. Bitwise equal to ops/pcg.py, sums by their order only.
//
// pcg_start ("pcg_start"): cg_start's residual into the core of r (no first
// direction). Last workgroup: rr, linf, rz = pq = alpha = beta = 0, iteration =
// 0, status.
template <typename T>
void pcg_start(const T* u, const T* g, T* r, const TileGeom& geom, Stencil5Coeffs c, PcgScalars* scalars,
               double* partials, unsigned* counter, hipStream_t s, GhostSides sides = {});
// pcg_apply ("pcg_apply"): cg_apply with z = M r in place of r: p_new =
// fma(T(beta), p_old, z) and the same q. Last workgroup: pq, alpha = rz / pq if
// pq > 0 and finite, otherwise alpha = 0 and status = 3.
template <typename T>
void pcg_apply(const T* z, const T* p_old, T* p_new, T* q, const TileGeom& geom, Stencil5Coeffs c, PcgScalars* scalars,
               double* partials, unsigned* counter, hipStream_t s, GhostSides sides = {});
// pcg_update ("pcg_update"): cg_update's expressions. Last workgroup: rr, linf,
// ++iteration, status; beta is not written (the dot epilogue owns it).
template <typename T>
void pcg_update(T* u, T* r, const T* p, const T* q, const TileGeom& geom, PcgScalars* scalars, double* partials,
                unsigned* counter, hipStream_t s);

// ------------------------------------------- implicit heat steps (kernels/cg.hip)
// The start of one theta-scheme step (heat.hpp; docs/ARCHITECTURE.md "Implicit
// heat steps"): cg_start / pcg_start with the step's right-hand side made in the
// same pass over u. With S = (n + s) + (w + e), ghosts as cg_start reads them
// (a mirror ghost is edge + ring), and the coefficients rounded to T once:
//   g = fma(T(b), S, T(a) c);  with a source  g = g + T(s) q  (product rounded, then the sum)
//   r = (fma(T(c1), S, T(0) c) + g) - c
// so r, rr and linf are bit for bit those of cg_start on (u, the stored g) with
// weights (0, c1): same grid, same partials. Writes the cores of g and r (and p
// = r for cg_heat_start); reads u with its ring and the core of q. q == nullptr
// selects the no-source kernels, which never read q. The last workgroup
// finishes the scalar block as cg_start / pcg_start do. ("cg_heat_start",
// "pcg_heat_start" in last_cg_dispatch().)
template <typename T>
void cg_heat_start(const T* u, const T* q, T* g, T* r, T* p, const TileGeom& geom, const HeatCoeffs& hc,
                   CgScalars* scalars, double* partials, unsigned* counter, hipStream_t s, GhostSides sides = {});
template <typename T>
void pcg_heat_start(const T* u, const T* q, T* g, T* r, const TileGeom& geom, const HeatCoeffs& hc,
                    PcgScalars* scalars, double* partials, unsigned* counter, hipStream_t s, GhostSides sides = {});

// The preconditioner's kernels: the multigrid kernels for any size, with the
// reflecting ghost of pcg.hpp. reflect_rows: the ghost row `height` reads as
// minus core row height - 1 (the ring row there is never read); reflect_cols
// likewise for column `width`. With both flags off and odd sides each gives the
// bits of its mg_* namesake. Each is bitwise equal to its reference in
// ops/pcg.py.
//
// Sides (`sides`, cg.hpp's GhostSides): a level's four ghost codes. Reflect
// (-1, far sides only) is the flag of before: the ghost is minus the edge cell.
// Mirror (+1, any side) is plus the edge cell, kept by the same mechanism: the
// thread that advances an edge cell writes the ghost beside it. In the
// transfers a mirror side also clamps the prolongation's coarse index (the
// coarse ghost equals the mirrored coarse cell) and doubles the fine residual
// of the row / column whose outer coarse neighbour is that ghost, so that
// 4 R = P^T still holds (docs/ARCHITECTURE.md "Neumann sides").
//
// mgp_smooth ("mgp_smooth"): mg_smooth with the flags: after every fused sweep
// the staged ghost row / column of a reflecting side becomes the negated new
// last core row / column (valid to the depth of the cell it mirrors). With
// `scalars` (then partials and counter too: 2 * mgp_smooth_grid_size(g) doubles
// and the CG ticket) the launch also sums src * u_out over the core in double,
// fma(double(src), double(out), acc), and its last workgroup writes rz' = the
// sum, beta = rz' / rz (0 while iteration == 0) and rz = rz' unless status != 0.
// u_in == nullptr ("mgp_smooth_zero"): the iterate starts at 0 and no tile is
// read for it; the bits are those of a launch on a zeroed u_in.
int mgp_smooth_grid_size(const TileGeom& g);
template <typename T>
void mgp_smooth(const T* u_in, T* u_out, const T* src, const TileGeom& g, const MgSweepTable& t, GhostSides sides,
                PcgScalars* scalars, double* partials, unsigned* counter, hipStream_t s);
// mgp_residual_restrict ("mgp_residual_restrict"): mg_residual_restrict for a
// coarse tile of (width / 2) x (height / 2): fine residuals outside the core
// count as 0 (on an even side the last coarse cell's far neighbours), and the
// residual reads the reflected ghost of a reflecting FINE level. The expression
// and order of mg_residual_restrict.
template <typename T>
void mgp_residual_restrict(const T* u, const T* src, const TileGeom& g, GhostSides sides, T* coarse_src,
                           const TileGeom& gc, Stencil5Coeffs c, hipStream_t s);
// mgp_prolong_add ("mgp_prolong_add"): mg_prolong_add's kernel (e = 0 outside
// the coarse core by index) for a coarse tile of (width / 2) x (height / 2).
template <typename T>
void mgp_prolong_add(const T* e, const TileGeom& gc, T* u, const TileGeom& g, hipStream_t s, GhostSides sides = {});
// mgp_coarse_solve ("mgp_coarse_solve"): mg_coarse_solve with the flags: the
// ghost row / column of a reflecting side is minus the last core row / column
// at every sweep (minus zero at the start). With `scalars` (a single-level
// preconditioner) it also sums src * e and writes rz and beta as mgp_smooth does.
template <typename T>
void mgp_coarse_solve(const T* src, T* e, const TileGeom& g, const MgSweepTable& t, int repeats, GhostSides sides,
                      PcgScalars* scalars, hipStream_t s);
const char* last_pcg_dispatch();

// Whether work on stream b runs while a kernel on stream a still runs (the two
// sit on different hardware queues): one bounded ~0.8 ms sleeping wave on a, a
// no-op kernel on b (kernels/queue_probe.hip). Synchronises both streams.
bool streams_concurrent(hipStream_t a, hipStream_t b);
// One single-wave kernel that holds stream s for `us` microseconds (capped at
// 10 ms) of the GPU's constant-rate wall clock (kernels/queue_probe.hip): the
// wire time an RCCL-loopback rehearsal adds after each transfer.
void spin_delay(double us, hipStream_t s);
// kClockStampWgs triples (XCD << 16 | SE/SH/CU id, shader clock counter — SCLK
// cycles, its rate follows DVFS —, constant-rate wall clock) at out[3 b ..],
// one per one-wave workgroup: two stamps around a launch, matched CU by CU,
// give the clock the launch ran at (device pointer).
constexpr int kClockStampWgs = 512;
void clock_stamp(unsigned long long* out, hipStream_t s);
// Number of 32-bit words that differ between a and b (bytes % 4 == 0) into
// *out (device pointer, overwritten): the direct halo's bitwise validation.
void count_diff(const void* a, const void* b, index_t bytes, unsigned* out, hipStream_t s);

// Update an arbitrary core rectangle [x0, x1) x [y0, y1) (scalar path; used for the
// boundary columns of the overlapped schedule and for tiny tiles).
template <typename T>
void stencil5_rect(const T* in, T* out, const TileGeom& g, index_t x0, index_t x1, index_t y0,
                   index_t y1, Stencil5Coeffs c, hipStream_t s);

// Processes sharing this GPU (ranks of one node bound to the same device, the
// IPC configuration). The persistent stencil kernels size their grid to the
// resident capacity of the chip divided by this, so the kernels of all sharing
// ranks are co-resident instead of queueing in rounds behind each other.
void set_gpu_share(int processes);
int gpu_share();

// Joint stage-1 windows in the fp32 two-stage pipeline (stencil_pipe_kernels.hpp:
// JointShape): on by default for time blocks that split into two multiples of
// 4 levels (S = 20, 24, 28, 32); off runs the per-strip layout (bitwise equal
// output). MXS_PIPE_JOINT=0 in the environment turns it off at start-up.
void set_pipe_joint(bool on);
bool pipe_joint();
// Ascending level order (one row of lag per level) in the joint pipeline where
// it measured faster: fp32 S = 20 and 24, fp64 S = 16 (pipe_form.hpp:
// pipe_form_for). Bitwise equal output.
// MXS_PIPE_LAG1=0 in the environment turns it off at start-up.
void set_pipe_lag1(bool on);
bool pipe_lag1();
// Whether the most recent stencil launch was a pipeline pass in that order.
bool last_pipe_lag1();
// The split narrow last column group of the fp32 S = 24 (12 + 12, ascending)
// pipeline pass (stencil_pipe_kernels.hpp: pipe_split_form; default on): when at most
// 440 columns are left for the last joint group, its workgroups run it as two
// two-strip sub-groups on half the rows each, so it costs half a group per row
// (32768 wide: 36.5 group-rows per row instead of 37). Off runs it as a whole
// four-strip group. Bitwise equal output. MXS_PIPE_SPLIT=0 in the environment
// turns it off at start-up.
void set_pipe_split(bool on);
bool pipe_split();
// Whether the most recent stencil launch was a pipeline pass that split its
// last group.
bool last_pipe_split();
// In-block progress priority of the fp32 S = 20 / 24 joint pipeline passes in
// ascending order, sum and scaled forms (stencil_pipe_kernels.hpp: pipe_chunk BPRIO;
// pipe_form.hpp: pipe_form_for; default on): the two
// waves that share a SIMD and a block barrier set their priority from the
// row's position inside the block, so neither parks at the barrier while the
// other finishes alone. Off runs the same kernels at equal priority. Bitwise
// equal output. A setter only: no start-up variable.
void set_pipe_block_prio(bool on);
bool pipe_block_prio();
// Whether the most recent stencil launch was a pipeline pass (one launch or
// chunk list) that ran with it.
bool last_pipe_block_prio();
// The four switches above as pipe_form_for() takes them.
PipeSwitches pipe_switches();
// The form of the most recent stencil launch if it was a pipeline pass (one
// launch or chunk list), else PipeForm{}: one record with
// last_stencil_dispatch(), last_pipe_lag1(), last_pipe_split() and
// last_pipe_block_prio().
PipeForm last_pipe_form();
// Fill-aware workgroup shares of the pipeline passes (chunk_schedule.hpp:
// balanced_starts; default on): a share that crosses a column-group boundary
// pays a second pipeline fill, and with equal row shares those workgroups set
// the pass time. MXS_PIPE_BALANCED=0 restores equal shares. Bitwise equal output.
void set_pipe_balanced(bool on);
bool pipe_balanced_on();

// Kernel form chosen by the most recent stencil launcher on this host process:
// "stream_pipe" (the two-stage pipeline: fp32 blocks > 16 steps, the one the
// benchmarks time, and fp64 blocks of 12 / 16 on whole lane vectors), "stream_balanced_rot" (persistent single-wave fp32
// rotated-pair kernel), "stream_balanced", "stream_grid_rot", "stream_grid", "tb_tile",
// "roll", "roll_wrap", "lds", "rect", "box", or a level-table pass:
// "stream_pipe_levels" (pipeline) or "held_levels" (held tile). A record of the host-side
// dispatch decision, for tests and result records; graph replays do not update it.
const char* last_stencil_dispatch();

// (2R+1)^2 box stencil with arbitrary weights (row-major, (2R+1)^2 entries), R in {1, 2}.
// Needs a ghost ring of at least R cells. LDS-tiled: each workgroup stages a
// (64+2R) x (16+2R) input tile once and reads the (2R+1)^2 taps from LDS.
constexpr int kMaxBoxRadius = 2;
struct BoxWeights {
  int radius = 1;
  float w[(2 * kMaxBoxRadius + 1) * (2 * kMaxBoxRadius + 1)] = {};
};
template <typename T>
void stencil_box(const T* in, T* out, const TileGeom& g, index_t x0, index_t x1, index_t y0,
                 index_t y1, const BoxWeights& w, hipStream_t s);

// ------------------------------------------------------ halo pack/unpack (K11/K12)
// A batch of strided 2D copies between up to three base pointers
// (slot 0 = tile, 1 = send buffer, 2 = recv buffer). One launch moves every
// segment of a halo exchange: gridDim.y indexes the copy.
constexpr int kMaxCopies = 24;
struct Copy2D {
  index_t src_off = 0, src_stride = 0;
  index_t dst_off = 0, dst_stride = 0;
  index_t width = 0, height = 0;
  int src_slot = 0, dst_slot = 0;
};
struct Copy2DBatch {
  int n = 0;
  Copy2D op[kMaxCopies];
};
// grid_x: workgroups per copy (0 = sized from the largest copy; tuning only).
// block: threads per workgroup (0 = 256). One-wave (64) workgroups are the
// ones the hardware places beside a running pipeline workgroup (the
// interior-first super-step's copies); 256 is faster alone.
// kind: which kernel symbol the launch uses (same body): halo_pack_kernel,
// halo_unpack_kernel or copy2d_batch_kernel, so kernel traces separate the
// exchange's two sides.
enum class CopyKind : int { Copy = 0, Pack = 1, Unpack = 2 };
template <typename T>
void copy2d_batch(T* slot0, T* slot1, T* slot2, const Copy2DBatch& b, hipStream_t s, int grid_x = 0, int block = 0,
                  CopyKind kind = CopyKind::Copy);

// ---------------------------------------------------------------- dot (K2-K8)
enum class DotReduce : int {
  Atomic = 0,      // per-block partial, one device atomic per block (mpicuda2.cu:65-81)
  TwoPass = 1,     // per-block partials + 1-block finisher kernel (mpicuda4.cu:71-88 + device finish)
  SinglePass = 2,  // last-block-done reduction with agent-scope release/acquire (mpicuda4.cu:157-185)
  HostPartials = 3,  // per-block partials, summed on the host in f64 (REDUCE_CPU)
  Racy = 4,        // NO_SYNC demonstrator: non-atomic `*out += partial` (ref_parallel-dot-product-atomics.cu:26-32)
};

// Scratch needed by the dot kernels: `partials` holds >= grid Acc values
// (dot_grid_size(n, kDotBlock) when grid <= 0: one workgroup per CU), `counter`
// one unsigned int (zeroed by the launcher every call).
int dot_grid_size(index_t n, int block);
constexpr int kDotBlock = 256;

// result = sum(x[i] * y[i]) accumulated in Acc (double or float). Writes the
// scalar into *out (device pointer). For HostPartials the partials are left in
// `partials[0..grid)` and *out is not written.
template <typename T, typename Acc>
void dot(const T* x, const T* y, index_t n, Acc* out, Acc* partials, unsigned* counter,
         DotReduce mode, int grid, hipStream_t s);

}  // namespace kernels
}  // namespace mxs
