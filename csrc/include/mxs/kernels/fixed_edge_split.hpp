// Fixed (non-periodic) edges under time blocking: which sides of a tile hold
// boundary values, and the split of its core into the part the S-step kernels
// can advance as they are and the frame that needs the held-side kernel
// (kernels::stencil5_tb_held). Host-only: shared by the kernel launchers, the
// solver and the _mxs_core bindings.
//
// After S steps a held side has influenced only the cells within S of it: an
// interior shrunk by S on every held side reads no held cell at any level, so
// it runs on the unchanged stencil5_tb kernels (any evaluation form). What is
// left, a frame S cells thick along the held sides, goes to the held kernel.
#pragma once

#include "mxs/core/config.hpp"

namespace mxs {
namespace kernels {

// Sides of a tile whose outside cells are boundary values: rows < 0 (top),
// rows >= height (bottom), columns < 0 (left), columns >= width (right).
enum HoldSide : unsigned { kHoldTop = 1, kHoldBottom = 2, kHoldLeft = 4, kHoldRight = 8 };

// Core rectangle [x0, x1) x [y0, y1).
struct Rect {
  index_t x0 = 0, x1 = 0, y0 = 0, y1 = 0;
  bool empty() const { return x1 <= x0 || y1 <= y0; }
};

struct FixedEdgeSplit {
  Rect interior;
  int n_frame = 0;
  Rect frame[4];
};

// The w x h core at depth S: `interior` is the core shrunk by S on the held
// sides only (left and right to whole `vec`-cell vectors, the rounding of the
// overlap schedule's strips: S rounded up on the left, w - S rounded down on
// the right), `frame` the rest in at most 4 disjoint rectangles: top and bottom
// strips over the full width, left and right strips between them. A core of at
// most 2S cells on a held axis has no interior: one frame rectangle is the
// whole core. interior + frame partition the core.
inline FixedEdgeSplit fixed_edge_split(index_t w, index_t h, int S, int vec, unsigned hold) {
  FixedEdgeSplit out;
  if (w <= 0 || h <= 0) return out;
  if (vec < 1) vec = 1;
  if (S < 0) S = 0;
  Rect in;
  in.y0 = (hold & kHoldTop) ? S : 0;
  in.y1 = (hold & kHoldBottom) ? h - S : h;
  in.x0 = (hold & kHoldLeft) ? (index_t(S) + vec - 1) / vec * vec : 0;
  in.x1 = (hold & kHoldRight) ? (w >= S ? (w - S) / vec * vec : 0) : w;
  if (in.empty()) {
    out.n_frame = 1;
    out.frame[0] = Rect{0, w, 0, h};
    return out;
  }
  out.interior = in;
  if (in.y0 > 0) out.frame[out.n_frame++] = Rect{0, w, 0, in.y0};
  if (in.y1 < h) out.frame[out.n_frame++] = Rect{0, w, in.y1, h};
  if (in.x0 > 0) out.frame[out.n_frame++] = Rect{0, in.x0, in.y0, in.y1};
  if (in.x1 < w) out.frame[out.n_frame++] = Rect{in.x1, w, in.y0, in.y1};
  return out;
}

}  // namespace kernels
}  // namespace mxs
