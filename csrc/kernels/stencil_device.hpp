// Device-side templates of the stencil kernels (included by stencil.hip and by
// the tuning harness bench/stencil_tune.hip so both compile the same code).
// See stencil.hip for the design notes. All of it is mxs::kernels::detail:
//   stencil_bodies.hpp        jac, lane moves, the Body* register layouts, strip shapes
//   stencil_sweep.hpp         one-step kernels: roll, lds, rect, box
//   stencil_tile.hpp          the single-buffer LDS tile (stencil5_tb1_kernel)
//   stencil_stream.hpp        single-wave streaming kernels; WavePrio, chunk_out_rsrc, RowFetch
//   stencil_pipe_kernels.hpp  the two-stage pipeline: pipe_chunk and its kernels
#pragma once

#include "stencil_bodies.hpp"
#include "stencil_pipe_kernels.hpp"
#include "stencil_stream.hpp"
#include "stencil_sweep.hpp"
#include "stencil_tile.hpp"
