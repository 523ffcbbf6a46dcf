// Two-stage pipeline instantiations, fp32 S = 17..32,
// per-step and sum form, wrap (1x1 periodic) and ghost-ring forms.
#include "stencil_pipe.hpp"

namespace mxs {
namespace kernels {
namespace detail {

template <typename T, int S, bool WRAP, EvalForm EF>
void launch_pipe(const T* in, T* out, const TileGeom& g, index_t x0, index_t x1, index_t y0, index_t y1, T c0, T c1,
                 hipStream_t s) {
  launch_pipe_impl<T, S, WRAP, EF>(in, out, g, x0, x1, y0, y1, c0, c1, s);
}

#define MXS_INST_LAUNCH(S, WRAP, EF)                                                                               \
  template void launch_pipe<float, S, WRAP, EvalForm::EF>(const float*, float*, const TileGeom&, index_t, index_t, \
                                                          index_t, index_t, float, float, hipStream_t);
#define MXS_INST_PIPE(S, EF)     \
  MXS_INST_LAUNCH(S, true, EF)   \
  MXS_INST_LAUNCH(S, false, EF)
#define MXS_INST_PIPE2(S)    \
  MXS_INST_PIPE(S, PerStep)  \
  MXS_INST_PIPE(S, Sum)

MXS_INST_PIPE2(17)
MXS_INST_PIPE2(18)
MXS_INST_PIPE2(19)
MXS_INST_PIPE2(20)
MXS_INST_PIPE2(21)
MXS_INST_PIPE2(22)
MXS_INST_PIPE2(23)
MXS_INST_PIPE2(24)
MXS_INST_PIPE2(25)
MXS_INST_PIPE2(26)
MXS_INST_PIPE2(27)
MXS_INST_PIPE2(28)
MXS_INST_PIPE2(29)
MXS_INST_PIPE2(30)
MXS_INST_PIPE2(31)
MXS_INST_PIPE2(32)

// The scaled form (any c_center, c_neighbor != 0) at the solver's depths.
MXS_INST_PIPE(20, Scaled)
MXS_INST_PIPE(24, Scaled)

#undef MXS_INST_PIPE2
#undef MXS_INST_PIPE
#undef MXS_INST_LAUNCH

}  // namespace detail
}  // namespace kernels
}  // namespace mxs
