"""The in-block progress priority of the fp32 pipeline passes
(stencil_pipe_kernels.hpp: pipe_chunk BPRIO; kernels::set_pipe_block_prio) under test.

Priority must be invisible in the field: every case runs the same solver with
the switch on and off and compares the two bitwise; the sum-form cases also
compare bitwise against ops.jacobi_sum_reference_global on the CPU, pass by
pass. Shapes: 2048 = two whole 904-column groups of the 12 + 12 pass plus 240
columns (the split two-strip sub-group path); 1824 and 1100 at S = 20 (two
groups, and a partial last group that is not split; tiles this narrow run
8 + 12, so a 12288-wide ghost-ring tile adds 12 + 8); the chunk-list pass
through a loopback solver in the peers' schedule; one per-step case. No
wall-clock or rate assertions.
"""
import pytest
import torch

from cuda_mpi_scratch_amd import hip
from cuda_mpi_scratch_amd.models.stencil2d import Stencil2D, StencilConfig
from cuda_mpi_scratch_amd.ops import jacobi_sum_reference_global


def _run(on, runs, **cfg):
    """The field after `runs` with the switch at `on`, the start field and what
    the last launch recorded."""
    H = hip()
    old = H.pipe_block_prio()
    try:
        H.set_pipe_block_prio(on)
        st = Stencil2D(StencilConfig(dims="1x1", dtype="f32", **cfg))
        u0 = st.core_view().clone()
        for n in runs:
            st.run(n)
        st.synchronize()
        return st.core_view().clone(), u0, H.last_stencil_dispatch(), H.last_pipe_form(), st
    finally:
        H.set_pipe_block_prio(old)


def _sum_reference(u0, S, passes):
    ref = u0.cpu()
    for _ in range(passes):
        ref = jacobi_sum_reference_global(ref, S)
    return ref


def test_switch_default_and_record():
    """CPU: on by default, the setter round-trips, and last_pipe_form() carries
    the field."""
    H = hip()
    assert H.pipe_block_prio() is True
    try:
        H.set_pipe_block_prio(False)
        assert H.pipe_block_prio() is False
    finally:
        H.set_pipe_block_prio(True)
    assert H.pipe_block_prio() is True
    form = H.last_pipe_form()
    assert "block_prio" in form and isinstance(form["block_prio"], bool)
    assert H.last_pipe_block_prio() == form["block_prio"]


@pytest.mark.gpu
@pytest.mark.parametrize("w,S,steps,js0,split", [
    (2048, 24, 24, 12, True),   # 2 x 904 + 240: the last group runs as two two-strip sub-groups
    (2048, 24, 48, 12, True),   # two passes
    (1824, 20, 20, 8, False),   # two groups (S = 20 runs 8 + 12 below 12288 columns: 928 + 896)
    (1100, 20, 20, 8, False),   # a partial last group that is not split
])
def test_periodic_sum_form_bitwise(gpu, w, S, steps, js0, split):
    kw = dict(global_width=w, global_height=1024, seed=w + steps, time_block=S)
    on, u0, kernel, form, st = _run(True, (steps,), **kw)
    assert st.time_block == S and kernel == "stream_pipe_sum"
    assert form["block_prio"] is True and form["lag1"] == 3 and form["js0"] == js0 and form["split"] == split, form
    off, u0_off, kernel, form, _ = _run(False, (steps,), **kw)
    assert kernel == "stream_pipe_sum" and form["block_prio"] is False and form["split"] == split, form
    assert torch.equal(u0, u0_off)
    assert torch.equal(on, off)
    assert torch.equal(on.cpu(), _sum_reference(u0, S, steps // S))


@pytest.mark.gpu
def test_ghost_ring_12_plus_8_bitwise(gpu):
    """12 + 8 proper (tiles from 12288 columns up take it, narrower ones 8 + 12):
    one S = 20 pass over a 12288 x 256 ghost-ring tile (13 groups of 912 columns
    and a partial one), on against off, through the kernel launcher."""
    from cuda_mpi_scratch_amd import core

    H = hip()
    S, w, h = 20, 12288, 256
    g = core().TileGeom.aligned(w, h, S, S, 4)
    src = torch.rand(g.alloc_elems(), generator=torch.Generator(device=gpu).manual_seed(w), device=gpu)
    outs = []
    old = H.pipe_block_prio()
    try:
        for on in (True, False):
            H.set_pipe_block_prio(on)
            dst = torch.full_like(src, -3.0)
            H.stencil5_tb(src.data_ptr(), dst.data_ptr(), g, S, 0, w, 0, h, 0.2, 0.2, False, "f32",
                          torch.cuda.current_stream().cuda_stream, "auto", True)
            form = H.last_pipe_form()
            assert H.last_stencil_dispatch() == "stream_pipe_sum"
            assert form["js0"] == 12 and form["block_prio"] is on, form
            torch.cuda.synchronize()
            outs.append(dst)
    finally:
        H.set_pipe_block_prio(old)
    assert torch.equal(outs[0], outs[1])


@pytest.mark.gpu
def test_chunk_list_pass_bitwise(gpu):
    """The same 2048 x 1024 tile through the chunk-list pass: a loopback solver
    in the peers' schedule opens interior-first (two launches of the chunk-list
    kernel). Bitwise the serial schedule's field, and on against off."""
    kw = dict(global_width=2048, global_height=1024, seed=17, time_block=24, backend="rccl", loopback=True)
    peers = dict(opening="interior-first", rehearse_peers=True, **kw)
    on, u0, kernel, form, st = _run(True, (24,), **peers)
    assert st.solver.halo_last(24) and kernel == "stream_pipe_sum_chunks"
    assert form["block_prio"] is True and form["js0"] == 12, form
    off, _, kernel, form, _ = _run(False, (24,), **peers)
    assert kernel == "stream_pipe_sum_chunks" and form["block_prio"] is False, form
    serial, _, kernel, _, _ = _run(True, (24,), opening="serial", **kw)
    assert kernel == "stream_pipe_sum"
    assert torch.equal(on, off)
    assert torch.equal(on, serial)
    assert torch.equal(on.cpu(), _sum_reference(u0, 24, 1))


@pytest.mark.gpu
def test_per_step_form_bitwise(gpu):
    """sum_form=False at S = 24: the per-step bodies keep equal priorities
    whatever the switch says, and stay bitwise 24 single steps."""
    kw = dict(global_width=2048, global_height=1024, seed=5, sum_form=False)
    on, _, kernel, form, _ = _run(True, (24,), time_block=24, **kw)
    assert kernel == "stream_pipe" and form["block_prio"] is False and form["js0"] == 12, form
    off, _, kernel, form, _ = _run(False, (24,), time_block=24, **kw)
    assert kernel == "stream_pipe" and form["block_prio"] is False, form
    one, _, _, _, _ = _run(True, (24,), time_block=1, **kw)
    assert torch.equal(on, off)
    assert torch.equal(on, one)
