"""One pipeline form for the one-launch and the chunk-list pass.

``stencil5_tb`` and ``stencil5_chunk_pass`` take their form (stage split, level
order, evaluation form) from the same rule (kernels/pipe_form.hpp:
pipe_form_for) through the same instantiation table (stencil_pipe.hpp:
with_pipe_form). Over the same ghost-ring tile they must therefore report the
same form and write the same bits, in each evaluation form, on both sides of
the fp32 S = 20 stage-split boundary (12288 columns) and at the other two
depths with chunk-list kernels. The tiles are the smallest whose chunk schedule
has an interior (256 rows: inner and outer workgroups > 0 at 256 workgroups).
"""
import pytest
import torch

from cuda_mpi_scratch_amd import core, hip

pytestmark = pytest.mark.gpu

# (c_center, c_neighbor, sum_form, range, kernel suffix). The inputs lie in
# [0, 1): range 1 keeps the scaled form (k = 4: growth 8^S) inside its bound.
FORMS = {
    "per_step": (0.2, 0.2, False, -1.0, ""),
    "sum": (0.2, 0.2, True, -1.0, "_sum"),
    "scaled": (0.5, 0.125, True, 1.0, "_scaled"),
}


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("w,h,S,dtype,js0", [
    (12284, 256, 20, "f32", 8),   # below the stage-split boundary: 8 + 12
    (12288, 256, 20, "f32", 12),  # from it: 12 + 8
    (2816, 256, 24, "f32", 12),
    (2816, 256, 16, "f64", 8),
])
def test_one_launch_and_chunk_pass_share_their_form(gpu, w, h, S, dtype, js0, form):
    c0, c1, sum_form, rng, suffix = FORMS[form]
    H = hip()
    tdt = torch.float32 if dtype == "f32" else torch.float64
    g = core().TileGeom.aligned(w, h, S, S, tdt.itemsize)
    gen = torch.Generator(device=gpu).manual_seed(w + S)
    src = torch.rand(g.alloc_elems(), generator=gen, device=gpu, dtype=torch.float64).to(tdt)
    ref = torch.full_like(src, -3.0)
    got = torch.full_like(src, -3.0)
    s = torch.cuda.current_stream().cuda_stream
    H.stencil5_tb(src.data_ptr(), ref.data_ptr(), g, S, 0, w, 0, h, c0, c1, False, dtype, s, "auto", sum_form, rng)
    assert H.last_stencil_dispatch() == "stream_pipe" + suffix
    one = H.last_pipe_form()
    d = H.stencil5_chunk_pass(src.data_ptr(), got.data_ptr(), g, S, c0, c1, dtype, 0, s, sum_form, rng)
    assert d is not None and d["check"] == "" and d["inner_blocks"] > 0 and d["outer_blocks"] > 0
    assert H.last_stencil_dispatch() == "stream_pipe" + suffix + "_chunks"
    assert (one["js0"], one["lag1"]) == (d["js0"], d["lag1"]) == (js0, 3)
    assert (H.last_pipe_form()["js0"], H.last_pipe_form()["lag1"]) == (js0, 3)
    torch.cuda.synchronize()
    assert torch.equal(got, ref)
