// The two-stage wave pipeline: pipe_chunk and its two kernels (one contiguous
// share per workgroup, or a chunk list). Launchers: stencil_pipe.hpp.
//
// WRITTEN OUT ON PURPOSE. The per-row level loop appears about a dozen times:
// ascending and descending order, warm-up and main loop, stage 0 and stage 1
// of pipe_chunk, and stream_chunk_fast (stencil_stream.hpp). So do the zero
// fill of the windows and the stage and write-out loops of the LDS tiles
// (stencil_tile.hpp, stencil_held.hpp). Moving them behind anything that
// receives the window array changes the generated code (gfx950 -S output
// compared per kernel with scripts/isa_same.py, nothing timed):
//   * win[3][L] passed to a function by reference, held in a struct member, or
//     captured by a local lambda: 0 of 27 chunk-list kernels keep their opcode
//     sequence, VGPR counts move by up to 7, 24 v_add_f32_dpp per kernel un-fold
//     into v_mov_b32_dpp + v_add, some kernels gain v_writelane SGPR spills;
//   * only the zero fill in a clear_window(win): 9 of 27 chunk-list kernels
//     and 296 of 364 kernels of stencil.hip keep their opcode sequence;
//   * one write-out function for stencil5_tb1_kernel and stencil5_tb_held_kernel:
//     0 of 144 held kernels and 268 of 364 of stencil.hip keep theirs.
// What is shared (set_wave_prio, chunk_out_rsrc, RowFetch, block_barrier,
// jac_vec) left every kernel's opcode sequence and register counts alone.
// Whoever tries again proves it with scripts/isa_same.py and a GPU measurement
// of every pipeline form.
//
// SHARED OVER THE COEFFICIENT SOURCE. None of the above forbids one kernel for
// several coefficient sources: the source is a kernel argument read through
// level_coeff (stencil_bodies.hpp), the window arrays stay where they are. Like
// pipe_chunk, two kernels are templates over it:
//   * the held tile (stencil_held.hpp), over T or LevelArray<T, S> and an
//     optional correction tile: 144 uniform, 12 level and 12 level + corr
//     kernels;
//   * the share walk of the level pipeline (stencil_pipe_levels.hpp), over
//     LevelPairs<T, S> or LevelPairsSrc<T, S>: 11 + 11 kernels.
// Each is, line for line, the kernel that was written out per source before
// (isa_same.py --pair, profiles/held_unify/isa_same.txt). Two spellings of the
// optional correction pointer were not harmless:
//   * a trailing argument of an empty "no corr" struct type instead of the
//     empty parameter pack: .amdhsa_kernarg_size grows by 4 on the 156 kernels
//     without a correction;
//   * the pack's pointer without __restrict__: the scalar loads of the 12 corr
//     kernels change.
// The uniform stencil5_stream_pipe_kernel keeps its own share walk (one
// __forceinline__ body for it and the level kernel reordered the scalar
// prologue of all 162 one-launch kernels, docs/PERF.md), and stencil5_tb1_kernel
// its own write-out (above).
#pragma once

#include "stencil_stream.hpp"

namespace mxs::kernels::detail {

// ------------------------------------------------- two-stage wave pipeline
// Deeper time blocks without more registers per wave. A single wave holds a
// three-slot window per level (12 VGPRs per level at fp32), so S = 16 already
// needs ~237 VGPRs; S = 20 in one wave drops to 1 wave per SIMD and spills to
// AGPRs, measured 35-45% slower per iteration (profiles/r02_deep). Here a
// column strip is streamed by TWO waves of the workgroup: stage 0 runs levels
// 1..S0 on rows fetched from HBM and hands each level-S0 row to stage 1
// through an LDS ring (one ds_write_b128 / ds_read_b128 per lane and row);
// stage 1 runs levels S0+1..S0+S1 and stores. Each wave keeps only its own
// levels' windows, so S = S0 + S1 reaches 20-32 at 2 waves per SIMD, and HBM
// sees one read + one write per cell per S iterations.
//
// Lock-step: all 8 waves of the workgroup (4 strips x 2 stages) advance in
// blocks of PF iterations with one barrier per block. Stage 0 emits its k-th
// output row at its iteration 3*S0 - 1 + k; stage 1 starts T1 blocks later and
// consumes row k at its iteration k, so every row it reads was written at
// least one barrier earlier; a ring of 3*PF rows per strip is never
// overwritten before it is read (see the derivation in docs/PERF.md). Both
// stages run the same number of blocks (their extra iterations read / write
// rows outside every stored cell's dependency cone). The apron is that of a
// single S-level wave (the strip's edge contamination spreads one column per
// level through both stages): OW = 256 - 2 * SA(S) output columns per strip.
template <int S0, int S1, int PF>
struct PipeShape {
  static constexpr int S = S0 + S1;
  static constexpr int RING = 3 * PF;                      // rows per strip in the LDS ring
  static constexpr int T1 = (3 * S0 + PF - 1 + PF - 1) / PF;  // stage-1 start block: ceil((3*S0 + PF - 1) / PF)
};

// Joint stage-1 windows (JOINT): JointShape, mxs/kernels/pipe_form.hpp.

// SUB (joint windows): the chunk may be one of several sub-groups of gs <= G
// strips that share the workgroup and its barriers (the split narrow group of
// stencil5_stream_pipe_kernel). `strip` then counts within the sub-group, `ring`
// points at the sub-group's first slot of the (G-strip) ring row, and the chunk
// runs the blocks of a chunk of sync_rows >= ye - ys rows; the extra iterations
// store nothing (the row term drops them) and read only clamped or wrapped
// rows. ye == ys is allowed. The caller passes wave-uniform values as such
// (wave_uniform): with a row range the compiler takes for per-lane, stage 0's
// row stepping moves to the VALU (+5% VALU per row, and the pass then ends
// 4% later, with the workgroups of the split group).
//
// In-block progress priority (BPRIO != 0). Every SIMD holds one stage-0 and one
// stage-1 wave of the workgroup, and both meet at the barrier that ends each
// block of PF rows. At equal priority the VALU arbiter prefers the older wave,
// which then runs its block ahead, parks at the barrier and leaves its partner
// to finish alone at the lower single-wave issue rate. With BPRIO a wave sets
// its priority from the row's position inside the block (block_prio_row), high
// at the block's first rows and low at its last, so the wave that is behind
// outranks the wave that is ahead and both reach the barrier together. Main
// loops only; a wave leaves the chunk at priority 0. s_setprio neither changes
// a result nor blocks a wave.
// BPRIO packs the levels, two bits per row: row k of a block runs at
// (BPRIO >> (12 * stage + 2 * k)) & 3 (kPipeBlockPrio: the production schedule).
//
// STAMP (tuner): s_memtime at arrival at and release from each main-loop
// barrier, summed per wave into *stamps (cycles parked, cycles in the bodies).
//
// C: the coefficient source (stencil_bodies.hpp: level_coeff). B::T, the
// default, is a uniform coefficient; a level table (stencil_pipe_levels.hpp)
// hands level l of the pass, counted over both stages, its own pair. The level
// index is a constant in every unrolled level loop below, and with C = B::T the
// kernels compile to the instructions they had before the parameter existed
// (scripts/isa_same.py). A source that carries a correction tile (CoeffCorr,
// stencil_bodies.hpp: the source term) makes stage 1 load the tile's cells at
// the store's offsets and add them to the row it stores; every other source
// compiles as before.
struct BlockStamps {
  unsigned long long parked = 0, body = 0;
};
constexpr unsigned pack_block_prio(int a0, int a1, int a2, int a3, int a4, int a5) {
  return unsigned(a0 | a1 << 2 | a2 << 4 | a3 << 6 | a4 << 8 | a5 << 10);
}
constexpr unsigned kPipeBlockPrio = pack_block_prio(3, 2, 2, 1, 1, 0) * 0x1001u;  // both stages alike
constexpr int block_prio_level(unsigned sched, int stage, int k) { return int(sched >> (12 * stage + 2 * k)) & 3; }
// Before row k of a block: the block's first row always sets its level (the
// wave may come from the warm-up at 0), later rows only where it changes.
template <unsigned BPRIO, int STAGE>
__device__ __forceinline__ void block_prio_row(int k) {
  if constexpr (BPRIO != 0) {
    if (k == 0 || block_prio_level(BPRIO, STAGE, k) != block_prio_level(BPRIO, STAGE, k - 1))
      set_wave_prio(block_prio_level(BPRIO, STAGE, k));
  }
}
// The barrier that ends a main-loop block; STAMP adds its two timestamps.
template <bool STAMP>
__device__ __forceinline__ void block_barrier(BlockStamps* stamps, unsigned long long& released) {
  if constexpr (STAMP) {
    const unsigned long long arrived = __builtin_amdgcn_s_memtime();
    __syncthreads();
    const unsigned long long now = __builtin_amdgcn_s_memtime();
    stamps->body += arrived - released;
    stamps->parked += now - arrived;
    released = now;
  } else {
    __syncthreads();
  }
}

template <typename B, int S0, int S1, int PF, bool WRAP, bool JOINT = false, int G = kWavesPerBlock, int LAG1 = 0,
          bool SUB = false, unsigned BPRIO = 0, bool STAMP = false, typename C = typename B::T>
__device__ __forceinline__ void pipe_chunk(const typename B::T* __restrict__ in, typename B::T* __restrict__ out,
                                           index_t pitch, index_t core_off, index_t W, index_t H, index_t xw,
                                           index_t x_end, index_t ys, index_t ye, const C c0, const C c1,
                                           typename B::V* __restrict__ ring, int stage, int strip = 0,
                                           index_t sync_rows = 0, int gs = G, BlockStamps* stamps = nullptr) {
  static_assert(BPRIO == 0 || PF <= 6, "a block-priority schedule packs six rows per stage");
  static_assert(!SUB || JOINT, "sub-groups are cut from joint windows");
  static_assert(PF % 3 == 0, "the window rotates through 3 slots: PF must be a multiple of 3");
  using P = PipeShape<S0, S1, PF>;
  constexpr int S = P::S, RING = P::RING;
  using T = typename B::T;
  using V = typename B::V;
  using Sh = StripShape<T, S, true>;
  using J = JointShape<S0, S1, G>;
  // Level order within a row iteration. Default: levels descend, so every
  // level reads only rows of earlier iterations (S independent evaluations per
  // row, level l lags 3 rows per level: a stage emits its first valid row at
  // iteration 3 * levels - 1). LAG1: levels ascend and each reads the row its
  // lower level made in the same iteration (a dependent chain per row), so a
  // level lags one row and a stage emits its first row at iteration 2 * levels:
  // S - 1 fewer fill iterations per chunk and stage. Same arithmetic per cell.
  // LAG1 is a stage mask: bit 0 = stage 0 ascends, bit 1 = stage 1 ascends.
  constexpr bool ASC0 = (LAG1 & 1) != 0, ASC1 = (LAG1 & 2) != 0;
  constexpr int E0 = ASC0 ? 2 * S0 : 3 * S0 - 1, E1 = ASC1 ? 2 * S1 : 3 * S1 - 1;
  constexpr int N = Sh::N, SA = Sh::SA, AL = SA / N;
  static_assert(!JOINT || N == 4, "joint windows assume 4-cell lanes");
  const int lane = threadIdx.x & (kWaveSize - 1);
  // Per-strip layout: xw = the strip's first output column, both stages cover
  // [xw - SA, xw - SA + 256). Joint: xw = the GROUP's first output column;
  // stage-0 wave `strip` covers [xw - LEAD + strip OW0, + 256), stage-1 wave
  // `strip` the window [xw - A1 + strip OW1, + 256).
  const index_t gx = JOINT ? (stage == 0 ? xw - J::LEAD + index_t(strip) * J::OW0 : xw - J::A1 + index_t(strip) * J::OW1) +
                                 index_t(lane) * N
                           : xw - SA + index_t(lane) * N;
  const index_t rows = ye - ys;
  // Stage 0 starts D rows early so that its ring writes start block-aligned
  // (row k is emitted at iteration 3*S0 - 1 + D + k, a multiple of PF for k = 0):
  // no per-row slot wrap. The lead rows only feed level-S0 rows before ys - S1.
  constexpr int D = (PF - E0 % PF) % PF;
  constexpr int T1 = (E0 + D) / PF + 1;  // stage-1 start block (P::T1 for the default order)
  static_assert(ASC0 || T1 == P::T1, "stage-1 start block");
  const index_t brows = SUB ? sync_rows : rows;  // the rows that set the block count
  // Valid columns of this (sub-)group's joint row and its output columns (JointShape, for gs strips).
  const int span = SUB ? gs * J::OW0 : J::SPAN;
  const int owg = SUB ? (span - 2 * J::A1 < gs * J::OW1 ? span - 2 * J::A1 : gs * J::OW1) : J::OWG;
  const index_t n_it0 = brows + 2 * S1 + E0 + D;  // stage 0: level-S0 rows [ys - S1, ye + S1)
  const index_t n_it1 = brows + E1;               // stage 1: output rows [ys, ye)
  const index_t blocks0 = (n_it0 + PF - 1) / PF, blocks1 = T1 + (n_it1 + PF - 1) / PF;
  const index_t blocks = blocks0 > blocks1 ? blocks0 : blocks1;
  // This lane's slot in a ring row, and the ring's row stride (lane vectors).
  constexpr int RSTRIDE = JOINT ? J::ROW : kWaveSize;
  int slot = lane;
  if constexpr (JOINT) {
    constexpr int AL0 = J::A0 / 4;  // stage-0 lanes per side without a valid level-S0 column
    if (stage == 0) {
      const bool valid = lane >= AL0 && lane < kWaveSize - AL0;
      const int tail = span / 4 + strip * 2 * AL0 + (lane < AL0 ? lane : lane - (kWaveSize - 2 * AL0));
      slot = valid ? strip * (J::OW0 / 4) + lane - AL0 : tail;
    } else {
      slot = strip * (J::OW1 / 4) + lane;
    }
  }
  V* __restrict__ my = ring + slot;

  if (stage == 0) {  // wave-uniform
    index_t lx;
    if (!JOINT && xw >= x_end) {
      lx = 0;  // idle strip past the rectangle: any valid address, nothing it makes is stored
    } else if constexpr (WRAP) {
      // Joint groups read up to G * 256 columns past their first output column.
      if (W >= (JOINT ? G : 1) * kWaveSize * N) lx = gx < 0 ? gx + W : (gx >= W ? gx - W : gx);
      else lx = ((gx % W) + W) % W;
    } else {
      const index_t last_col = (W + N - 1) / N * N + SA - N;
      lx = gx < last_col ? gx : last_col;
    }
    const T* __restrict__ pin = in + core_off + lx;
    const index_t last_row = ye + S - 1;
    // The first PF rows (the D lead rows clamped to the first needed row when
    // there is no wrap: they may lie above the ghost ring; wrapped twice on a
    // torus of fewer than S + D rows, H >= S > D, where one wrap leaves them
    // above row 0).
    V pf[PF];
#pragma unroll
    for (int k = 0; k < PF; ++k) {
      index_t r = ys - S - D + k;
      if constexpr (WRAP) {
        r = r < 0 ? r + H : r;
        if constexpr (D > 0) r = r < 0 ? r + H : r;
      } else {
        r = r < ys - S ? ys - S : r;
      }
      pf[k] = B::load(pin + r * pitch);
    }
    index_t first = ys - S - D + PF;
    if constexpr (WRAP) first = first < 0 ? first + H : first;
    RowFetch<B, WRAP> fetch(pin, pitch, WRAP ? H : last_row, first);
    V win[3][S0];
#pragma unroll
    for (int q = 0; q < 3; ++q)
#pragma unroll
      for (int l = 0; l < S0; ++l) win[q][l] = B::zero();
    // See stream_chunk_fast: level l matters from iteration 3l + 2 (LAG1: 2l).
    constexpr int kWarm = ASC0 ? (2 * S0) / PF * PF : (3 * (S0 - 1)) / PF * PF;
#pragma unroll 1
    for (int ib = 0; ib < kWarm; ib += PF) {
#pragma unroll
      for (int k = 0; k < PF; ++k) {
        if constexpr (ASC0) {
          const int n = k % 3, o = (k + 1) % 3, m = (k + 2) % 3;  // rows of iterations j, j-2, j-1
          const int b = (ib + k) / 2;
          win[n][0] = B::enter(pf[k]);
          pf[k] = fetch();
#pragma unroll
          for (int l = 0; l < S0 - 1; ++l)
            if (l < b) win[n][l + 1] = B::jac(win[o][l], win[m][l], win[n][l], level_coeff(c0, l), level_coeff(c1, l));
        } else {
          const int p0 = k % 3, p1 = (k + 1) % 3, p2 = (k + 2) % 3;
          const int b = (ib + k) / 3;
          win[p2][0] = B::enter(pf[k]);
          pf[k] = fetch();
#pragma unroll
          for (int l = S0 - 2; l >= 0; --l)
            if (l <= b)
              win[p0][l + 1] = B::jac(win[p0][l], win[p1][l], win[p2][l], level_coeff(c0, l), level_coeff(c1, l));
        }
      }
      __syncthreads();
    }
    // Ring slot of each block's first row k = i - (3*S0 - 1): a wave-uniform
    // counter stepping by PF modulo RING (a 64-bit modulo per block cost ~40
    // scalar instructions).
    int base = ((kWarm - (E0 + D)) % RING + RING) % RING;  // 0, PF or 2 PF
    unsigned long long released = 0;
    if constexpr (STAMP) released = __builtin_amdgcn_s_memtime();
#pragma unroll 1
    for (index_t i = kWarm; i < blocks * PF; i += PF) {
#pragma unroll
      for (int k = 0; k < PF; ++k) {
        block_prio_row<BPRIO, 0>(k);
        V top;
        if constexpr (ASC0) {
          const int n = k % 3, o = (k + 1) % 3, m = (k + 2) % 3;
          win[n][0] = B::enter(pf[k]);
          pf[k] = fetch();
#pragma unroll
          for (int l = 0; l < S0; ++l) {
            const V v = B::jac(win[o][l], win[m][l], win[n][l], level_coeff(c0, l), level_coeff(c1, l));
            if (l == S0 - 1) top = v;
            else win[n][l + 1] = v;
          }
        } else {
          const int p0 = k % 3, p1 = (k + 1) % 3, p2 = (k + 2) % 3;
          win[p2][0] = B::enter(pf[k]);
          pf[k] = fetch();
#pragma unroll
          for (int l = S0 - 1; l >= 0; --l) {
            const V o = B::jac(win[p0][l], win[p1][l], win[p2][l], level_coeff(c0, l), level_coeff(c1, l));
            if (l == S0 - 1) top = o;
            else win[p0][l + 1] = o;
          }
        }
        // Row k = j - (3*S0 - 1 + D) of stage 1's input (rotated layout);
        // writes for k < 0 land in slots no reader touches before they are
        // rewritten. base + k < RING: blocks are ring-aligned.
        my[(base + k) * RSTRIDE] = top;
        if constexpr (B::kStage0Fence) __builtin_amdgcn_sched_barrier(0);
      }
      base = base + PF < RING ? base + PF : 0;
      block_barrier<STAMP>(stamps, released);
    }
    if constexpr (block_prio_level(BPRIO, 0, PF - 1) != 0) __builtin_amdgcn_s_setprio(0);
  } else {
    // Output descriptor over rows [ys, ye) (see stream_chunk_fast).
    const index_t x0w = gx - index_t(lane) * N;  // the window's first column
    const __amdgpu_buffer_rsrc_t orsrc = chunk_out_rsrc(out + core_off + x0w + ys * pitch, rows, pitch);
    // A correction tile (CoeffCorr): the same descriptor over it, read at the store's offsets.
    constexpr bool CORR = CoeffCorr<C>::value;
    __amdgpu_buffer_rsrc_t crsrc;
    if constexpr (CORR) crsrc = chunk_out_rsrc(coeff_corr(c0) + core_off + x0w + ys * pitch, rows, pitch);
    bool store_lane;
    if constexpr (JOINT) {
      // Inside this window's own apron and inside the group's output span
      // [A1, A1 + OWG) (the last window may run past it); windows tile the group.
      constexpr int AL1 = J::A1 / 4;
      const int q = strip * J::OW1 + lane * N;  // joint-row column of this lane's first cell
      store_lane = lane >= AL1 && lane < kWaveSize - AL1 && q + N <= J::A1 + owg && gx < x_end;
    } else {
      store_lane = lane >= AL && lane < kWaveSize - AL && gx < x_end && xw < x_end;
    }
    // Store offset = lane term + row term, both past the range when dropped: a
    // dropped lane adds 2^31, a dropped row 0x7F000000 (chunks are at most
    // kMaxChunkBytes = 0x7F000000 bytes, so no sum wraps past 2^32 and every
    // sum with a dropped term is >= the range). The row term is wave-uniform
    // (scalar select), so a row costs one v_add_u32 (a 64-bit v_cmp and a
    // v_cndmask per row before).
    const unsigned lane_term = store_lane ? unsigned(lane) * unsigned(N * sizeof(T)) : 0x80000000u;
    const unsigned row_bytes = unsigned(pitch) * unsigned(sizeof(T));
    const int rows_i = int(rows);
    V win[3][S1];
#pragma unroll
    for (int q = 0; q < 3; ++q)
#pragma unroll
      for (int l = 0; l < S1; ++l) win[q][l] = B::zero();
#pragma unroll 1
    for (int t = 0; t < T1; ++t) __syncthreads();  // stage 0 fills the ring
    constexpr int kWarm = ASC1 ? (2 * S1) / PF * PF : (3 * (S1 - 1)) / PF * PF;
#pragma unroll 1
    for (int ib = 0; ib < kWarm; ib += PF) {
      V inrow[PF];
      const int base = (ib / PF) % 3 * PF;  // RING = 3 * PF and ib is a multiple of PF
#pragma unroll
      for (int k = 0; k < PF; ++k) inrow[k] = my[(base + k) * RSTRIDE];
#pragma unroll
      for (int k = 0; k < PF; ++k) {
        if constexpr (ASC1) {
          const int n = k % 3, o = (k + 1) % 3, m = (k + 2) % 3;
          const int b = (ib + k) / 2;
          win[n][0] = inrow[k];
#pragma unroll
          for (int l = 0; l < S1 - 1; ++l)
            if (l < b)
              win[n][l + 1] = B::jac(win[o][l], win[m][l], win[n][l], level_coeff(c0, S0 + l), level_coeff(c1, S0 + l));
        } else {
          const int p0 = k % 3, p1 = (k + 1) % 3, p2 = (k + 2) % 3;
          const int b = (ib + k) / 3;
          win[p2][0] = inrow[k];
#pragma unroll
          for (int l = S1 - 2; l >= 0; --l)
            if (l <= b)
              win[p0][l + 1] =
                  B::jac(win[p0][l], win[p1][l], win[p2][l], level_coeff(c0, S0 + l), level_coeff(c1, S0 + l));
        }
      }
      __syncthreads();
    }
    int base = (kWarm / PF) % 3 * PF;  // ring slot of the block's first row (counter, see stage 0)
    unsigned long long released = 0;
    if constexpr (STAMP) released = __builtin_amdgcn_s_memtime();
#pragma unroll 1
    for (index_t i = kWarm; i < (blocks - T1) * PF; i += PF) {
      V inrow[PF];
#pragma unroll
      for (int k = 0; k < PF; ++k) inrow[k] = my[(base + k) * RSTRIDE];
      base = base + PF < RING ? base + PF : 0;
#pragma unroll
      for (int k = 0; k < PF; ++k) {
        block_prio_row<BPRIO, 1>(k);
        const index_t j = i + k;
        V top;
        // The row's correction first: its latency falls behind the S1 levels.
        CorrRow<T> cv;
        if constexpr (CORR) {
          const int rc = int(j - E1);
          corr_load(cv, crsrc, lane_term + (rc >= 0 && rc < rows_i ? unsigned(rc) * row_bytes : unsigned(kMaxChunkBytes)));
        }
        if constexpr (ASC1) {
          const int n = k % 3, o = (k + 1) % 3, m = (k + 2) % 3;
          win[n][0] = inrow[k];
#pragma unroll
          for (int l = 0; l < S1; ++l) {
            const V v = B::jac(win[o][l], win[m][l], win[n][l], level_coeff(c0, S0 + l), level_coeff(c1, S0 + l));
            if (l == S1 - 1) top = v;
            else win[n][l + 1] = v;
          }
        } else {
          const int p0 = k % 3, p1 = (k + 1) % 3, p2 = (k + 2) % 3;
          win[p2][0] = inrow[k];
#pragma unroll
          for (int l = S1 - 1; l >= 0; --l) {
            const V o = B::jac(win[p0][l], win[p1][l], win[p2][l], level_coeff(c0, S0 + l), level_coeff(c1, S0 + l));
            if (l == S1 - 1) top = o;
            else win[p0][l + 1] = o;
          }
        }
        const int r = int(j - E1);
        const unsigned row_term = r >= 0 && r < rows_i ? unsigned(r) * row_bytes : unsigned(kMaxChunkBytes);
        if constexpr (CORR) corr_store(top, cv, orsrc, lane_term + row_term);
        else B::store(top, orsrc, lane_term + row_term, level_coeff(c0, 0));
      }
      block_barrier<STAMP>(stamps, released);
    }
    if constexpr (block_prio_level(BPRIO, 1, PF - 1) != 0) __builtin_amdgcn_s_setprio(0);
  }
}

// Balanced persistent launch of the two-stage pipeline: 512-thread workgroups
// (4 strips x 2 stages), equal shares of (4-strip group) x rows as in
// stencil5_stream_balanced_kernel. T = float: rotated-pair layout; T = double:
// wide-lane body (FastBody<T>). Needs x_end % 4 == 0 and a chunk of at most
// kMaxChunkBytes (the output buffer descriptor and its drop offsets).
// PRIO (tuning): 1 raises the fetching stage's wave priority, 2 the storing stage's.
// G: strips per workgroup (2G waves; the barriers of one block of rows span the
// workgroup, so smaller groups decouple the strips of a CU).
// XM (tuning): XCD-major share order — the workgroups one XCD runs (blockIdx
// congruent mod 8) take consecutive shares, so vertically adjacent chunks, which
// read the same 2S apron rows, share that XCD's L2.
// JOINT: joint stage-1 windows (JointShape), OWG output columns per group.
// Workgroup ranges of the linear (group x rows) space: equal shares of `share`
// rows (n == 0), or explicit fill-aware starts (kernels/chunk_schedule.hpp:
// balanced_starts), start[w] .. start[w + 1] for workgroup w — passed by value
// in the kernel arguments (2 KB), so a launch needs no device table and stays
// graph-capturable.
//
// The split narrow group. A partial last group costs a whole one: all eight
// waves stream every row of it whatever it stores (32768 columns at S = 24:
// 36.25 groups of 904, and the 37th stores 224 columns). When what is left for
// the last group fits a two-strip joint group (JointShape<S0, S1, 2>: 440
// columns at 12 + 12), the workgroup runs it as two independent two-strip
// sub-groups side by side: sub-group s = strip / 2 takes waves {strip % 2,
// stage}, half s of every ring row and half s of the rows, so the group costs
// half a group per row. In the linear space the group is split_half =
// ceil(rows / 2) long, and a workgroup holding [a, b) of it runs rows [a, b)
// on sub-group 0 and [a + half, min(b + half, rows)) on sub-group 1. Both take
// the same barriers (pipe_chunk SUB: the block count of sub-group 0's rows,
// never the fewer). Same operations per cell in the same order: bitwise equal
// output. fp32 12 + 12 in the ascending order only (the headline pass).
__device__ __forceinline__ int wave_uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ index_t wave_uniform(index_t v) {
  const unsigned long long u = static_cast<unsigned long long>(v);
  const unsigned lo = __builtin_amdgcn_readfirstlane(unsigned(u)), hi = __builtin_amdgcn_readfirstlane(unsigned(u >> 32));
  return index_t((static_cast<unsigned long long>(hi) << 32) | lo);
}
constexpr int kMaxShareBlocks = 512;
struct PipeShares {
  index_t share = 0;
  index_t split_half = 0;  // > 0: the last group is split and this long in the linear space
  int n = 0;
  int start[kMaxShareBlocks + 1];
  static PipeShares equal(index_t share) {
    PipeShares p;
    p.share = share;
    return p;
  }
};

template <int S0, int S1, int PF, bool WRAP, int PRIO = 0, typename T = float, bool SUM = false,
          int G = kWavesPerBlock, bool XM = false, bool JOINT = false, int LAG1 = 0, int XB = 0, unsigned BPRIO = 0>
__global__ __launch_bounds__(2 * G * kWaveSize) void stencil5_stream_pipe_kernel(
    const T* __restrict__ in, T* __restrict__ out, index_t pitch, index_t core_off, index_t W, index_t H,
    index_t x_begin, index_t x_end, index_t y_begin, index_t y_end, const PipeShares shares, T c0, T c1) {
  using P = PipeShape<S0, S1, PF>;
  using B = typename FastBody<T, SUM, XB>::type;
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
  if constexpr (PRIO == 1) {
    if (stage == 0) __builtin_amdgcn_s_setprio(1);
  } else if constexpr (PRIO == 2) {
    if (stage == 1) __builtin_amdgcn_s_setprio(1);
  }
  index_t slot = blockIdx.x;
  if constexpr (XM) {
    if (gridDim.x % kNumXcds == 0) slot = (blockIdx.x % kNumXcds) * (gridDim.x / kNumXcds) + blockIdx.x / kNumXcds;
  }
  index_t a, b;
  if (shares.n > 0) {
    a = shares.start[slot];
    b = shares.start[slot + 1];
  } else {
    a = slot * shares.share;
    b = a + shares.share < total ? a + shares.share : total;
  }
  // Rows per pipe_chunk call: its output buffer descriptor spans at most
  // kMaxChunkBytes (32-bit offsets), so on very wide tiles (rows of MiBs: a
  // 65536^2 fp32 tile, 16 GiB per buffer) a share is walked in pieces, each
  // paying its own pipeline fill (the launcher checks >= 64 rows fit).
  const index_t max_rows = kMaxChunkBytes / (pitch * index_t(sizeof(T)));
  if (max_rows < 1) return;  // workgroup-uniform, before any barrier (never launched so: the host checks)
#pragma unroll 1
  while (a < b) {  // workgroup-uniform: all 8 waves take every chunk (barriers inside)
    const index_t grp = a / rows, r0 = a - grp * rows;
    if constexpr (SPLIT) {
      if (half > 0 && grp == groups - 1) {  // workgroup-uniform
        // The split narrow group: [r0, r1) of its half rows on sub-group 0, the
        // same range of the other half on sub-group 1 (pieces per sub-group);
        // each sub-group's joint row is its half of the ring row.
        index_t r1 = half < r0 + (b - a) ? half : r0 + (b - a);
        r1 = r1 - r0 > max_rows ? r0 + max_rows : r1;
        // Wave-uniform, and told so: they depend on the wave's strip.
        const int sub = wave_uniform(strip / 2), sstrip = wave_uniform(strip % 2);
        const index_t q0 = wave_uniform(!sub ? r0 : r0 + half < rows ? r0 + half : rows);
        const index_t q1 = wave_uniform(!sub ? r1 : r1 + half < rows ? r1 + half : rows);
        using J = JointShape<S0, S1, G>;
        static_assert(JointShape<S0, S1, G / 2>::ROW * 2 == J::ROW, "a sub-group's joint row is half the ring row");
        pipe_chunk<B, S0, S1, PF, WRAP, true, G, LAG1, true, BPRIO>(in, out, pitch, core_off, W, H, x_begin + grp * OWG,
                                                                    x_end, y_begin + q0, y_begin + q1, c0, c1,
                                                                    ring + sub * (J::ROW / 2), stage, sstrip, r1 - r0,
                                                                    G / 2);
        a += r1 - r0;
        continue;
      }
    }
    index_t r1 = rows < r0 + (b - a) ? rows : r0 + (b - a);
    r1 = r1 - r0 > max_rows ? r0 + max_rows : r1;
    if constexpr (JOINT) {
      pipe_chunk<B, S0, S1, PF, WRAP, true, G, LAG1, false, BPRIO>(in, out, pitch, core_off, W, H, x_begin + grp * OWG,
                                                                   x_end, y_begin + r0, y_begin + r1, c0, c1, ring, stage,
                                                                   strip);
    } else {
      const index_t xw = x_begin + (grp * G + strip) * OW;
      pipe_chunk<B, S0, S1, PF, WRAP, false, G, LAG1, false, BPRIO>(in, out, pitch, core_off, W, H, xw, x_end,
                                                                    y_begin + r0, y_begin + r1, c0, c1,
                                                                    ring + strip * P::RING * kWaveSize, stage);
    }
    a += r1 - r0;
  }
}

// Chunk-list pass (kernels/chunk_schedule.hpp): the joint-window pipeline of
// stencil5_stream_pipe_kernel (ghost-ring tile, no wrap) over an explicit chunk
// list per workgroup instead of one contiguous share. The interior-first
// multi-GPU super-step runs two launches of it on disjoint CUs (core chunks
// beside the halo exchange, then the ghost-ring chunks). The halo copy kernel
// (copy2d_batch_kernel, 32 VGPRs) runs beside it: two pass waves per SIMD leave
// it 32 of the 512 VGPRs in the sum forms (fp32 12 + 8 / 12 + 12: 238, 8 + 12:
// 225, 8-VGPR granules; with the block priority 220 and 189); the per-step
// 8 + 12 and fp64 8 + 8 forms (244) leave 16, and their copies take the CUs the
// inner launch leaves free.
template <int S0, int S1, int PF, typename T, bool SUM, int LAG1, int XB = 0, unsigned BPRIO = 0>
__global__ __launch_bounds__(2 * kWavesPerBlock * kWaveSize) void stencil5_pipe_chunks_kernel(
    const T* __restrict__ in, T* __restrict__ out, index_t pitch, index_t core_off, index_t W, index_t H,
    index_t x_begin, index_t x_end, index_t y_begin, const PassChunk* __restrict__ table, int entries, T c0, T c1) {
  constexpr int G = kWavesPerBlock;
  using P = PipeShape<S0, S1, PF>;
  using B = typename FastBody<T, SUM, XB>::type;
  constexpr int OWG = JointShape<S0, S1, G>::OWG;
  __shared__ typename B::V ring[G * P::RING * kWaveSize];
  const int wave = threadIdx.x / kWaveSize;
  const int strip = wave % G, stage = wave / G;
  const PassChunk* __restrict__ mine = table + index_t(blockIdx.x) * entries;
  const index_t max_rows = kMaxChunkBytes / (pitch * index_t(sizeof(T)));  // pieces, as in stencil5_stream_pipe_kernel
  if (max_rows < 1) return;  // workgroup-uniform, before any barrier (chunk_pass_shape refuses such rows)
#pragma unroll 1
  for (int e = 0; e < entries; ++e) {  // workgroup-uniform
    const PassChunk c = mine[e];
    if (c.r1 <= c.r0) break;  // lists are packed from slot 0
#pragma unroll 1
    for (index_t r0 = c.r0; r0 < c.r1; r0 += max_rows) {
      const index_t r1 = c.r1 - r0 > max_rows ? r0 + max_rows : c.r1;
      pipe_chunk<B, S0, S1, PF, false, true, G, LAG1, false, BPRIO>(in, out, pitch, core_off, W, H,
                                                                    x_begin + index_t(c.group) * OWG, x_end, y_begin + r0,
                                                                    y_begin + r1, c0, c1, ring, stage, strip);
    }
  }
}

}  // namespace mxs::kernels::detail
