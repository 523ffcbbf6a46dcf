// Single-wave streaming kernels, and what they share with the two-stage pipeline:
// the wave priority switch, the output buffer descriptor, the fetching row cursor.
#pragma once

#include "stencil_bodies.hpp"

namespace mxs::kernels::detail {

// ------------------------------------------------------- wave-streaming blocks
// Temporal blocking without LDS and without vertical recompute. Each wave owns a
// column strip (64 lanes x one 16-byte vector = 256 fp32 / 128 fp64 columns, of
// which the outer SA columns per side are apron) and streams down a chunk of CH
// rows. It keeps a three-row window per time level in registers: when input row
// y arrives, level 1 row y-1 is computed from level-0 rows y-2..y, level 2 row
// y-2 from level-1 rows y-3..y-1, ..., level S row y-S is stored. Row neighbours
// come from the same lane's window; column neighbours from the adjacent lanes
// through ds_bpermute. Every level advances once per input row, so HBM sees one
// read and one write per cell per S steps (plus 2S/CH rows and 2SA/256 columns
// of redundant apron). The window is three register slots per level used
// round-robin (the loop is unrolled by a multiple of 3), so no row is ever
// copied between registers: VALU work is just the stencil arithmetic.
//
// One wave streams output rows [ys, ye) of the column strip whose first output
// column is xw. PF = input rows in flight (a register ring, statically indexed;
// a multiple of 3, the window's slot period).
//
// Skewed schedule: in iteration j level l works on the row level l-1 made in
// iteration j-1, so the S levels of one iteration are independent (S-way ILP
// instead of an S-long dependent chain of cross-lane move -> VALU). Slots per
// level rotate with the phase p = j % 3: up = win[p], mid = win[p+1],
// dn = win[p+2]; level l writes its output into win[p][l+1], the slot that is
// level l+1's dn next iteration, after level l+1 has read it as up (so levels
// run top-down). Level S-1 outputs row y_first + j - 2S + 1.
template <typename T, int S, int PF, bool WRAP, bool DPP>
__device__ __forceinline__ void stream_chunk(const T* __restrict__ in, T* __restrict__ out, index_t pitch,
                                             index_t core_off, index_t W, index_t H, index_t xw, index_t x_end,
                                             index_t ys, index_t ye, T c0, T c1) {
  static_assert(PF % 3 == 0, "the window rotates through 3 slots: PF must be a multiple of 3");
  using Sh = StreamShape<T, S>;
  constexpr int N = Sh::N, SA = Sh::SA, AL = SA / N;
  using V = typename Vec16<T>::type;
  const int lane = threadIdx.x & (kWaveSize - 1);
  const index_t gx = xw - SA + index_t(lane) * N;

  index_t lx = gx;
  bool load_ok = true;
  if constexpr (WRAP) {
    if (W >= kWaveSize * N) lx = gx < 0 ? gx + W : (gx >= W ? gx - W : gx);
    else lx = ((gx % W) + W) % W;
  } else {
    load_ok = gx < W + SA;  // inside the row padding of TileGeom::aligned
  }
  const T* __restrict__ pin = in + core_off + lx;
  const bool store_lane = lane >= AL && lane < kWaveSize - AL && gx < x_end;
  const bool full_vec = gx + N <= x_end;
  const int addr_l = ((lane + kWaveSize - 1) & (kWaveSize - 1)) << 2;
  const int addr_r = ((lane + 1) & (kWaveSize - 1)) << 2;

  // Next input row to fetch, as a (wrapped) row index.
  const index_t y_first = ys - S;
  index_t next = y_first;
  if constexpr (WRAP) next = next < 0 ? next + H : next;
  auto fetch = [&]() -> V {
    V v = V(T(0));
    if (load_ok) v = *reinterpret_cast<const V*>(pin + next * pitch);
    ++next;
    if constexpr (WRAP) next = next == H ? 0 : next;
    return v;
  };
  T* __restrict__ pout = out + core_off + gx + ys * pitch;  // first output row

  V win[3][S];
#pragma unroll
  for (int q = 0; q < 3; ++q)
#pragma unroll
    for (int l = 0; l < S; ++l) win[q][l] = V(T(0));

  const index_t n_in = (ye - ys) + 2 * S;
  const index_t n_it = (ye - ys) + 3 * S - 1;
  V pf[PF];
#pragma unroll
  for (int k = 0; k < PF; ++k) pf[k] = k < n_in ? fetch() : V(T(0));
#pragma unroll 1
  for (index_t i = 0; i < n_it; i += PF) {
#pragma unroll
    for (int k = 0; k < PF; ++k) {
      const index_t j = i + k;
      if (j < n_it) {
        const int p0 = k % 3, p1 = (k + 1) % 3, p2 = (k + 2) % 3;  // static after the unroll
        win[p2][0] = pf[k];
        if (j + PF < n_in) pf[k] = fetch();
        V top = V(T(0));
#pragma unroll
        for (int l = S - 1; l >= 0; --l) {
          const V m = win[p1][l];
          const T left = DPP ? lane_shift<T, kDppWaveShr1>(m[N - 1]) : lane_fetch<T>(m[N - 1], addr_l);
          const T right = DPP ? lane_shift<T, kDppWaveShl1>(m[0]) : lane_fetch<T>(m[0], addr_r);
          const V o = jac_row<T, V>(win[p0][l], m, win[p2][l], left, right, c0, c1);
          if (l == S - 1) top = o;
          else win[p0][l + 1] = o;
        }
        if (j >= 3 * S - 1 && store_lane) {  // row ys + (j - 3S + 1)
          T* p = pout + (j - (3 * S - 1)) * pitch;
          if (full_vec) {
            __builtin_nontemporal_store(top, reinterpret_cast<V*>(p));
          } else {
#pragma unroll
            for (int q = 0; q < N; ++q)
              if (gx + q < x_end) p[q] = top[q];
          }
        }
      }
    }
  }
}

// The wave's issue priority (WavePrio below, block_prio_row of the pipeline).
__device__ __forceinline__ void set_wave_prio(int level) {
  switch (level) {  // s_setprio takes an immediate
    case 3: __builtin_amdgcn_s_setprio(3); break;
    case 2: __builtin_amdgcn_s_setprio(2); break;
    case 1: __builtin_amdgcn_s_setprio(1); break;
    default: __builtin_amdgcn_s_setprio(0); break;
  }
}

// Progress-based wave priority (balanced launch). Two waves share each SIMD and
// the VALU arbiter prefers the older one, so with equal work the first-launched
// workgroup of a CU finished at ~62% of the kernel and its partner ran the last
// ~38% alone at ~70% of the paired issue rate (per-wave s_memrealtime stamps on
// 32768^2, TUNE_FOCUS=stamp of bench/stencil_tune). Each wave instead sets its
// priority from the fraction of its share still ahead of it (4 levels), so
// the laggard gets the issue slots and both finish together.
struct WavePrio {
  index_t done = 0;       // rows of the share finished before this chunk
  float quarters = 0.f;   // 4 / share rows (0: priority left alone)
  int level = -1;         // current level (s_setprio value)
};
__device__ __forceinline__ void wave_prio_update(WavePrio& wp, index_t done) {
  if (wp.quarters == 0.f) return;
  const float q = float(done) * wp.quarters;
  const int level = q >= 3.f ? 0 : (q >= 2.f ? 1 : (q >= 1.f ? 2 : 3));
  if (level == wp.level) return;
  wp.level = level;
  set_wave_prio(level);
}

// Buffer descriptor over a chunk's `rows` output rows from `obase` (wave-uniform,
// and told so): the branch-free stores of stream_chunk_fast and pipe_chunk go
// through it, and the hardware range check drops an offset past its range.
// `obase` is the first column of the wave's 256-column window, so the range
// ends with the window's last row: on a tile whose rows are shorter than the
// window (pitch < 256; a wrapping pass needs no row padding) that is past
// rows * pitch, and a range of rows * pitch dropped the last row's stores
// beyond column pitch of the window. Never more than kMaxChunkBytes, which the
// dropped offsets count on (only a piece of ~10^6 rows of such a tile gets there).
template <typename T>
__device__ __forceinline__ __amdgpu_buffer_rsrc_t chunk_out_rsrc(const T* obase, index_t rows, index_t pitch) {
  const unsigned long long ob = reinterpret_cast<unsigned long long>(obase);
  const unsigned ob_lo = __builtin_amdgcn_readfirstlane(unsigned(ob)),
                 ob_hi = __builtin_amdgcn_readfirstlane(unsigned(ob >> 32));
  T* obase_u = reinterpret_cast<T*>((static_cast<unsigned long long>(ob_hi) << 32) | ob_lo);
  constexpr index_t kWindow = 4 * kWaveSize;  // columns of a window: 4 cells per lane in both element types
  index_t elems = rows * pitch;
  if (pitch < kWindow && rows > 0) elems += kWindow - pitch;
  index_t bytes = elems * index_t(sizeof(T));
  bytes = bytes < kMaxChunkBytes ? bytes : kMaxChunkBytes;
  const int nbytes = __builtin_amdgcn_readfirstlane(int(bytes));
  return __builtin_amdgcn_make_buffer_rsrc(obase_u, 0, nbytes, 0x00020000);
}

// Row cursor of a fetching wave (stream_chunk_fast, pipe_chunk stage 0): a call
// loads the lane's vector of row `next` and steps on; the row wraps at the tile
// height (WRAP) or saturates at the last input row, so no fetch branches.
template <typename B, bool WRAP>
struct RowFetch {
  const typename B::T* __restrict__ pin;
  index_t pitch, lim;  // lim: the tile height under WRAP, else the last input row
  index_t next;        // the row the next call loads
  index_t roff;        // element offset of row `next`, stepped (no multiply per row)
  __device__ __forceinline__ RowFetch(const typename B::T* p, index_t row_pitch, index_t limit, index_t first_row)
      : pin(p), pitch(row_pitch), lim(limit), next(first_row), roff(first_row * row_pitch) {}
  __device__ __forceinline__ typename B::V operator()() {
    const typename B::V v = B::load(pin + roff);
    if constexpr (WRAP) {
      ++next;
      const bool wrap = next == lim;
      next = wrap ? 0 : next;
      roff = wrap ? 0 : roff + pitch;
    } else {
      const bool adv = next < lim;
      next = adv ? next + 1 : next;
      roff = adv ? roff + pitch : roff;
    }
    return v;
  }
};

// fp32 form of stream_chunk on the rotated-pair layout (jac_rot4f) with a
// branch-free row loop, so the whole unrolled PF-row body is ONE basic block:
// any branch inside it (a guarded fetch, an exec-masked store) lets the backend
// hoist the DPP shifts of the next row above it, and a v_mov_b32_dpp that is
// not in its consumer's block cannot fold into the add (measured: 96 separate
// v_mov_b32_dpp per 48 level-rows otherwise). Hence:
//   * fetches always load: the row index saturates at the last input row (or
//     wraps, WRAP) and lanes past the row padding read its last vector —
//     values that cannot reach a stored cell within S levels (a stored cell at
//     x < x_end <= W depends on inputs in [x - S, x + S] only, SA >= S);
//   * stores go through a buffer descriptor over this chunk's output rows, and
//     a lane/row that must not store gets an out-of-range offset, which the
//     buffer range check drops (no exec mask, no branch);
//   * the row count is rounded up to PF; the extra iterations store nothing.
// Needs x_end % 4 == 0 (whole vectors) and (ye - ys) * pitch * 4 < 2^31 bytes
// (checked by the launcher, which falls back to stream_chunk otherwise).
// Generic over the per-lane body B (BodyRotF32: rotated fp32, BodyWideF64: 4 fp64
// cells per lane). Non-WRAP reads need x_origin + halo_x >= SA (the launcher checks it).
template <typename B, int S, int PF, bool WRAP>
__device__ __forceinline__ void stream_chunk_fast(const typename B::T* __restrict__ in, typename B::T* __restrict__ out,
                                                  index_t pitch, index_t core_off, index_t W, index_t H, index_t xw,
                                                  index_t x_end, index_t ys, index_t ye, typename B::T c0,
                                                  typename B::T c1, WavePrio* wp = nullptr) {
  static_assert(PF % 3 == 0, "the window rotates through 3 slots: PF must be a multiple of 3");
  using T = typename B::T;
  using V = typename B::V;
  using Sh = StripShape<T, S, true>;
  constexpr int N = Sh::N, SA = Sh::SA, AL = SA / N;
  const int lane = threadIdx.x & (kWaveSize - 1);
  const index_t gx = xw - SA + index_t(lane) * N;

  index_t lx;
  if constexpr (WRAP) {
    if (W >= kWaveSize * N) lx = gx < 0 ? gx + W : (gx >= W ? gx - W : gx);
    else lx = ((gx % W) + W) % W;
  } else {
    const index_t last_col = (W + N - 1) / N * N + SA - N;  // last vector of the row padding
    lx = gx < last_col ? gx : last_col;
  }
  const T* __restrict__ pin = in + core_off + lx;

  // Output descriptor: rows [ys, ye) from column xw - SA (wave-uniform base).
  const index_t rows = ye - ys;
  const __amdgpu_buffer_rsrc_t orsrc = chunk_out_rsrc(out + core_off + (xw - SA) + ys * pitch, rows, pitch);
  const bool store_lane = lane >= AL && lane < kWaveSize - AL && gx < x_end;
  const unsigned lane_off = unsigned(lane) * unsigned(N * sizeof(T));
  const unsigned row_bytes = unsigned(pitch) * unsigned(sizeof(T));
  constexpr unsigned kDrop = 0x80000000u;  // >= nbytes: dropped by the range check

  index_t first = ys - S;
  if constexpr (WRAP) first = first < 0 ? first + H : first;
  RowFetch<B, WRAP> fetch(pin, pitch, WRAP ? H : ye + S - 1, first);

  V win[3][S];
#pragma unroll
  for (int q = 0; q < 3; ++q)
#pragma unroll
    for (int l = 0; l < S; ++l) win[q][l] = B::zero();

  const index_t n_it = rows + 3 * S - 1;
  V pf[PF];
#pragma unroll
  for (int k = 0; k < PF; ++k) pf[k] = fetch();
  // Warm-up: level l first produces a row any stored cell depends on at
  // iteration 3l + 2, so iteration block b (iterations 3b .. 3b+2) only runs
  // levels 0..b; the skipped levels would compute rows outside every stored
  // cell's dependency cone. The warm-up covers the whole PF-steps below
  // 3(S-1) (the first store is at 3S-1); it halves the warm-up work of the
  // (3S-1) extra iterations every chunk pays, 14% of a 292-row share of the
  // 8-GPU tile.
  constexpr int kWarm = (3 * (S - 1)) / PF * PF;
  if (wp) wave_prio_update(*wp, wp->done);
#pragma unroll 1
  for (int ib = 0; ib < kWarm; ib += PF) {
#pragma unroll
    for (int k = 0; k < PF; ++k) {
      const int p0 = k % 3, p1 = (k + 1) % 3, p2 = (k + 2) % 3;
      const int b = (ib + k) / 3;  // wave-uniform
      win[p2][0] = B::enter(pf[k]);
      pf[k] = fetch();
#pragma unroll
      for (int l = S - 2; l >= 0; --l) {
        if (l <= b) win[p0][l + 1] = B::jac(win[p0][l], win[p1][l], win[p2][l], c0, c1);
      }
    }
  }
#pragma unroll 1
  for (index_t i = kWarm; i < n_it; i += PF) {
    if (wp && (i & 63) == 0) wave_prio_update(*wp, wp->done + i);
#pragma unroll
    for (int k = 0; k < PF; ++k) {
      const index_t j = i + k;
      const int p0 = k % 3, p1 = (k + 1) % 3, p2 = (k + 2) % 3;  // static after the unroll
      if (j >= n_it) break;  // wave-uniform (scalar branch); without it the allocator spills to AGPRs
      win[p2][0] = B::enter(pf[k]);
      pf[k] = fetch();
      V top;
#pragma unroll
      for (int l = S - 1; l >= 0; --l) {
        const V o = B::jac(win[p0][l], win[p1][l], win[p2][l], c0, c1);
        if (l == S - 1) top = o;
        else win[p0][l + 1] = o;
      }
      const index_t r = j - (3 * S - 1);  // output row (relative to ys) of this iteration
      const bool ok = store_lane && r >= 0 && r < rows;
      const unsigned off = ok ? lane_off + unsigned(r) * row_bytes : kDrop;
      B::store(top, orsrc, off, c0);
    }
  }
}

// Grid form: workgroup = 4 waves on 4 adjacent strips of the same CH-row chunk.
// ROT: the branch-free 4-cells-per-lane body (stream_chunk_fast: rotated-pair
// fp32 or wide-lane fp64; the launcher checks its preconditions).
template <typename T, int S, int PF, bool WRAP, bool DPP = true, bool ROT = false>
__global__ __launch_bounds__(kBlock) void stencil5_stream_kernel(const T* __restrict__ in, T* __restrict__ out,
                                                                 index_t pitch, index_t core_off, index_t W, index_t H,
                                                                 index_t x_begin, index_t x_end, index_t y_begin,
                                                                 index_t y_end, index_t CH, T c0, T c1) {
  constexpr int OW = StripShape<T, S, ROT>::OW;
  const index_t xw = x_begin + (index_t(blockIdx.x) * kWavesPerBlock + threadIdx.x / kWaveSize) * OW;
  if (xw >= x_end) return;  // wave-uniform
  const index_t ys = y_begin + index_t(blockIdx.y) * CH;
  const index_t ye = ys + CH < y_end ? ys + CH : y_end;
  if constexpr (ROT)
    stream_chunk_fast<typename FastBody<T>::type, S, PF, WRAP>(in, out, pitch, core_off, W, H, xw, x_end, ys, ye, c0, c1);
  else stream_chunk<T, S, PF, WRAP, DPP>(in, out, pitch, core_off, W, H, xw, x_end, ys, ye, c0, c1);
}

// Balanced persistent form: exactly as many workgroups as fit on the chip at
// once. The work is (group of 4 adjacent strips) x rows, split into equal
// shares of rows per workgroup (group-major); a workgroup's 4 waves stream the
// 4 strips of its group over the same rows side by side — as in the grid form,
// so the apron columns two neighbouring waves both read are L2 hits — and a
// share that crosses a group boundary restarts there. No tail round, and
// (3S-1)/share redundant rows instead of (3S-1)/CH per chunk.
template <typename T, int S, int PF, bool WRAP, bool DPP = true, bool ROT = false, bool SUM = false, int XB = 0>
__global__ __launch_bounds__(kBlock) void stencil5_stream_balanced_kernel(
    const T* __restrict__ in, T* __restrict__ out, index_t pitch, index_t core_off, index_t W, index_t H,
    index_t x_begin, index_t x_end, index_t y_begin, index_t y_end, index_t share, T c0, T c1) {
  constexpr int OW = StripShape<T, S, ROT>::OW;
  const index_t rows = y_end - y_begin;
  const index_t strips = (x_end - x_begin + OW - 1) / OW;
  const index_t groups = (strips + kWavesPerBlock - 1) / kWavesPerBlock;
  const index_t total = groups * rows;
  const int wave = threadIdx.x / kWaveSize;
  index_t a = index_t(blockIdx.x) * share;
  const index_t a0 = a;
  const index_t b = a + share < total ? a + share : total;
  WavePrio wp;
  if (b > a) wp.quarters = 4.f / float(b - a);
  // ROT stores go through one buffer descriptor per call: longer shares are
  // walked in pieces of at most kMaxChunkBytes (see stencil5_stream_pipe_kernel).
  const index_t max_rows = ROT ? kMaxChunkBytes / (pitch * index_t(sizeof(T))) : rows;
  if (max_rows < 1) return;  // workgroup-uniform (rot_ok keeps such rows on the plain body)
#pragma unroll 1
  while (a < b) {  // workgroup-uniform
    const index_t grp = a / rows, r0 = a - grp * rows;
    index_t r1 = rows < r0 + (b - a) ? rows : r0 + (b - a);
    r1 = r1 - r0 > max_rows ? r0 + max_rows : r1;
    const index_t xw = x_begin + (grp * kWavesPerBlock + wave) * OW;
    if (xw < x_end) {
      wp.done = a - a0;
      if constexpr (ROT)
        stream_chunk_fast<typename FastBody<T, SUM, XB>::type, S, PF, WRAP>(in, out, pitch, core_off, W, H, xw, x_end,
                                                                        y_begin + r0, y_begin + r1, c0, c1, &wp);
      else
        stream_chunk<T, S, PF, WRAP, DPP>(in, out, pitch, core_off, W, H, xw, x_end, y_begin + r0, y_begin + r1, c0,
                                          c1);
    }
    a += r1 - r0;
  }
}

}  // namespace mxs::kernels::detail
