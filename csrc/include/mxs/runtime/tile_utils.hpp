// What the single-GPU Poisson solvers (MultigridSolver, CgSolver, PcgSolver) do
// alike with a tile of TileGeom::aligned(w, h, 1, 1): write boundary values into
// its ring and read the norms of the true residual back.
#pragma once

#include <cmath>

#include "mxs/kernels/kernels.hpp"
#include "mxs/runtime/hip_utils.hpp"

namespace mxs {

// Boundary values into the depth-1 ring of the device tile `u`: device pointers
// to width (top, bottom) or height (left, right) values, nullptr leaves a side
// as it is. Enqueued on `s`, not synchronised.
template <typename T>
void copy_ring_sides(T* u, const TileGeom& g, const T* top, const T* bottom, const T* left, const T* right,
                     hipStream_t s) {
  const index_t off = g.core_offset();
  if (top) MXS_HIP_CHECK(hipMemcpyAsync(u + off - g.pitch, top, size_t(g.width) * sizeof(T), hipMemcpyDeviceToDevice, s));
  if (bottom)
    MXS_HIP_CHECK(hipMemcpyAsync(u + off + g.height * g.pitch, bottom, size_t(g.width) * sizeof(T),
                                 hipMemcpyDeviceToDevice, s));
  if (left)
    MXS_HIP_CHECK(hipMemcpy2DAsync(u + off - 1, size_t(g.pitch) * sizeof(T), left, sizeof(T), sizeof(T), size_t(g.height),
                                   hipMemcpyDeviceToDevice, s));
  if (right)
    MXS_HIP_CHECK(hipMemcpy2DAsync(u + off + g.width, size_t(g.pitch) * sizeof(T), right, sizeof(T), sizeof(T),
                                   size_t(g.height), hipMemcpyDeviceToDevice, s));
}

// The buffers of a stencil5_residual read-back and the read-back itself.
struct ResidualReadback {
  DeviceBuffer<double> buf;  // the norms, then the partials
  DeviceBuffer<unsigned> counter;
  PinnedBuffer<double> host;

  void reset(const TileGeom& g) {
    buf.reset(2 + 2 * index_t(kernels::residual_grid_size(g)));
    counter.reset(1);
    host.reset(2);
  }
  // Norms of (A u + src) - u over the core, ring ghosts: R is {linf, l2, cells}. A synchronising read.
  template <typename R, typename T>
  R read(const T* u, const T* src, const TileGeom& g, double c_center, double c_neighbor, const Stream& stream) {
    auto* norms = reinterpret_cast<kernels::ResidualNorms*>(buf.get());
    const kernels::Stencil5Coeffs c{c_center, c_neighbor, false, -1.0};
    kernels::stencil5_residual<T>(u, g, c, norms, buf.get() + 2, counter.get(), stream.get(), src);
    MXS_HIP_CHECK(hipMemcpyAsync(host.get(), norms, sizeof(kernels::ResidualNorms), hipMemcpyDeviceToHost, stream.get()));
    stream.spin_sync();
    R r;
    r.linf = host.get()[0];
    r.l2 = std::sqrt(host.get()[1]);
    r.cells = g.width * g.height;
    return r;
  }
};

}  // namespace mxs
