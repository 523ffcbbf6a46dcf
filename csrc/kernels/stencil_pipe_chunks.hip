// Chunk-list pipeline pass of the interior-first multi-GPU super-step
// (kernels.hpp: chunk_pass_shape / stencil5_chunk_pass; device body
// stencil5_pipe_chunks_kernel in stencil_pipe_kernels.hpp; chunk lists
// kernels/chunk_schedule.hpp). Its form is the one pipe_form_for() gives the
// one-launch pass over the same ghost-ring tile, through the same table
// (stencil_pipe.hpp: with_pipe_form), so the split pass runs exactly the kernel
// body the one-launch pass runs. The joint forms of fp32 S = 20 and 24 and fp64
// S = 16 have chunk-list kernels, in every evaluation form; other depths and
// the per-strip layout keep the one-launch pass.
#include <type_traits>

#include "stencil_pipe.hpp"

namespace mxs {
namespace kernels {
namespace detail {
namespace {

// BP: with the in-block progress priority (pipe_block_prio_form forms only).
template <typename T, int S, EvalForm EF, int JS0, int LAG1, bool BP = false>
constexpr auto chunks_kernel() {
  static_assert(!BP || pipe_block_prio_form<T, JS0, S - JS0, true, LAG1, eval_sum(EF)>(),
                "no block-priority kernel in this form");
  return stencil5_pipe_chunks_kernel<JS0, S - JS0, kPerStrip<T, S, EF>.pf, T, eval_sum(EF), LAG1, eval_xb(EF),
                                     BP ? kPipeBlockPrio : 0u>;
}

// Calls fn(depth, form) with the compile-time depth and evaluation form; false
// when `steps` has no chunk-list kernels in element type T.
template <typename T, typename F>
bool with_chunk_depth(int steps, EvalForm eval, F&& fn) {
  auto forms = [&](auto depth) {
    if (eval == EvalForm::Scaled) fn(depth, std::integral_constant<EvalForm, EvalForm::Scaled>{});
    else if (eval == EvalForm::Sum) fn(depth, std::integral_constant<EvalForm, EvalForm::Sum>{});
    else fn(depth, std::integral_constant<EvalForm, EvalForm::PerStep>{});
    return true;
  };
  if constexpr (sizeof(T) == 4) {
    if (steps == 20) return forms(std::integral_constant<int, 20>{});
    if (steps == 24) return forms(std::integral_constant<int, 24>{});
  } else {
    if (steps == 16) return forms(std::integral_constant<int, 16>{});
  }
  return false;
}

}  // namespace
}  // namespace detail

template <typename T>
bool chunk_pass_shape(const TileGeom& g, int steps, const Stencil5Coeffs& c, ChunkPassShape* out) {
  using namespace detail;
  constexpr index_t N = 16 / index_t(sizeof(T));
  if (g.width % 4 != 0 || g.width < 4 * kWaveSize || g.height < 2 * steps) return false;
  if (g.halo_x < steps || g.halo_y < steps) return false;
  if ((g.pitch % N) != 0 || ((g.x_origin + g.halo_x) % N) != 0) return false;
  // Entries longer than kMaxChunkBytes run in pieces (stencil5_pipe_chunks_kernel).
  if (!chunk_rows_fit(g.pitch, sizeof(T))) return false;
  ChunkPassShape sh;
  bool ok = false;
  with_chunk_depth<T>(steps, eval_form<T>(c, steps), [&](auto depth, auto form) {
    constexpr int S = decltype(depth)::value;
    constexpr EvalForm EF = decltype(form)::value;
    const PipeChoice ch = pipe_form_for(int(sizeof(T)), S, EF, g.width, pipe_switches());
    if (!ch.form.joint) return;  // the per-strip layout has no chunk-list form
    const index_t lead = g.x_origin + g.halo_x, sa = pipe_apron(ch.form);
    if (lead < sa || g.pitch < lead + (g.width + 3) / 4 * 4 + sa) return;
    if (sizeof(T) == 8 && !wide_pipe_ok_impl<T, S, false>(g, 0, g.width)) return;
    with_pipe_form<T, S, EF>(ch, [&](auto tag) {
      using K = decltype(tag);
      if constexpr (K::JS0 > 0) {
        // Both fast forms share the sum-form kernel's shape.
        constexpr EvalForm kQuery = eval_sum(EF) ? EvalForm::Sum : EvalForm::PerStep;
        sh.blocks = resident_workgroups(reinterpret_cast<const void*>(chunks_kernel<T, S, kQuery, K::JS0, K::LAG1>()),
                                        2 * kBlock, 1);
      }
    });
    sh.steps = S;
    sh.form = ch.form;
    sh.eval = ch.eval;
    sh.owg = pipe_owg(ch.form);
    sh.groups = pipe_groups(ch.form, g.width);
    sh.fill = pipe_fill_rows(ch.form);
    sh.read_lead = sa;
    sh.read_span = pipe_read_span(ch.form);
    ok = true;
  });
  if (ok && out) *out = sh;
  return ok;
}

template <typename T>
void stencil5_chunk_pass(const T* in, T* out, const TileGeom& g, const Stencil5Coeffs& c, const ChunkPassShape& sh,
                         const PassChunk* table, int entries, hipStream_t s) {
  using namespace detail;
  MXS_CHECK(table != nullptr && entries > 0 && sh.blocks > 0, "stencil5_chunk_pass: no schedule");
  ChunkPassShape now;
  MXS_CHECK(chunk_pass_shape<T>(g, sh.steps, c, &now) && now.eval == sh.eval,
            "stencil5_chunk_pass: shape built for the other evaluation form");
  const bool known = with_chunk_depth<T>(sh.steps, sh.eval, [&](auto depth, auto form) {
    constexpr int S = decltype(depth)::value;
    constexpr EvalForm EF = decltype(form)::value;
    with_pipe_form<T, S, EF>(PipeChoice{sh.form, sh.eval}, [&](auto tag) {
      using K = decltype(tag);
      if constexpr (K::JS0 > 0) {
        const KernelCoeffs<T> k = kernel_coeffs(EF, T(c.center), T(c.neighbor), S);
        // The priority switch as it stands at this launch, like the one-launch pass.
        const bool block_prio = pipe_form_for(int(sizeof(T)), S, EF, g.width, pipe_switches()).block_prio;
        auto launch = [&](auto kernel) {
          kernel<<<sh.blocks, 2 * kBlock, 0, s>>>(in, out, g.pitch, g.core_offset(), g.width, g.height, 0, g.width, 0,
                                                  table, entries, k.a, k.b);
        };
        if constexpr (pipe_block_prio_form<T, K::JS0, S - K::JS0, true, K::LAG1, eval_sum(EF)>()) {
          if (block_prio) launch(chunks_kernel<T, S, EF, K::JS0, K::LAG1, true>());
          else launch(chunks_kernel<T, S, EF, K::JS0, K::LAG1>());
        } else {
          launch(chunks_kernel<T, S, EF, K::JS0, K::LAG1>());
        }
        note_launch(EF == EvalForm::Scaled ? "stream_pipe_scaled_chunks"
                    : EF == EvalForm::Sum  ? "stream_pipe_sum_chunks"
                                           : "stream_pipe_chunks",
                    sh.form, false, block_prio);
      } else {
        MXS_CHECK(false, "stencil5_chunk_pass: the per-strip layout has no chunk-list form");
      }
    });
  });
  MXS_CHECK(known, "stencil5_chunk_pass: no chunk-list kernels at depth " << sh.steps);
  MXS_HIP_CHECK_LAUNCH();
}

template bool chunk_pass_shape<float>(const TileGeom&, int, const Stencil5Coeffs&, ChunkPassShape*);
template bool chunk_pass_shape<double>(const TileGeom&, int, const Stencil5Coeffs&, ChunkPassShape*);
template void stencil5_chunk_pass<float>(const float*, float*, const TileGeom&, const Stencil5Coeffs&,
                                         const ChunkPassShape&, const PassChunk*, int, hipStream_t);
template void stencil5_chunk_pass<double>(const double*, double*, const TileGeom&, const Stencil5Coeffs&,
                                          const ChunkPassShape&, const PassChunk*, int, hipStream_t);

}  // namespace kernels
}  // namespace mxs
