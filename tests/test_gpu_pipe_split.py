"""The split narrow last column group of the fp32 S = 24 pipeline pass
(stencil_pipe_kernels.hpp: pipe_split_form) under test.

When at most 440 columns are left for the last joint group of a 12 + 12 pass,
its workgroups run it as two two-strip sub-groups on half the rows each. Every
check is bitwise, against the same pass with the split off (set_pipe_split) and
against the per-strip layout (set_pipe_joint off, documented bitwise equal);
the periodic sum form also against ops.jacobi_sum_reference_global. The shapes
sit on the split's edges: remainders of 4, 224 and 440 columns (split), 444 (not
split), a single narrow group, and row counts whose second half is empty (1),
unequal (7, 97) or several blocks of rows long.
"""
import pytest
import torch

from cuda_mpi_scratch_amd import core, hip
from cuda_mpi_scratch_amd.ops import jacobi_sum_reference_global

pytestmark = pytest.mark.gpu

S = 24
OWG, OWG2 = 904, 440  # output columns of a four-strip and of a two-strip 12 + 12 joint group
WIDTHS = (OWG + 224, OWG + OWG2, OWG + OWG2 + 4, OWG + 4, 224)
HEIGHTS = (1, 2, 7, 97, 192)
FORMS = {  # name: (c_center, c_neighbor, sum_form, range, dispatch record)
    "sum": (0.2, 0.2, True, -1.0, "stream_pipe_sum"),
    "step": (0.2, 0.2, False, -1.0, "stream_pipe"),
    "scaled": (0.3, 0.1, True, 1.0, "stream_pipe_scaled"),
}


def _splits(w):
    return w - (-(-w // OWG) - 1) * OWG <= OWG2


def _core(buf, g, w, h):
    return buf.view(g.total_height(), g.pitch)[g.halo_y:g.halo_y + h, g.x_origin + g.halo_x:g.x_origin + g.halo_x + w]


def _tile(gpu, w, h, wrap, seed):
    """A periodic tile of at least S rows whose rows [y0, y0 + h) are updated, or
    a ghost-ring tile of exactly w x h; random values everywhere, padding included."""
    th = max(h, 40) if wrap else h
    y0 = 5 if th > h else 0
    g = core().TileGeom.aligned(w, th, 1 if wrap else S, 1 if wrap else S, 4)
    gen = torch.Generator(device=gpu).manual_seed(seed)
    src = torch.rand(g.alloc_elems(), generator=gen, device=gpu, dtype=torch.float64).float()
    return g, src, th, (0, w, y0, y0 + h)


def _pass(src, g, rect, wrap, form, split=True, joint=True):
    H = hip()
    c0, c1, sum_form, rng, record = FORMS[form]
    x0, x1, y0, y1 = rect
    old = H.pipe_split(), H.pipe_joint()
    try:
        H.set_pipe_split(split)
        H.set_pipe_joint(joint)
        dst = torch.full_like(src, -3.0)
        H.stencil5_tb(src.data_ptr(), dst.data_ptr(), g, S, x0, x1, y0, y1, c0, c1, wrap, "f32",
                      torch.cuda.current_stream().cuda_stream, "auto", sum_form, rng)
        assert H.last_stencil_dispatch() == record
        did_split = H.last_pipe_split()
        torch.cuda.synchronize()
    finally:
        H.set_pipe_split(old[0])
        H.set_pipe_joint(old[1])
    return dst, did_split


def _check(gpu, w, h, wrap, form, joint_oracle=True):
    g, src, th, rect = _tile(gpu, w, h, wrap, seed=w * 7 + h)
    got, did = _pass(src, g, rect, wrap, form)
    assert did == _splits(x := rect[1] - rect[0]), (x, did)
    whole, did = _pass(src, g, rect, wrap, form, split=False)
    assert not did
    assert torch.equal(got, whole)
    if joint_oracle:
        strips, did = _pass(src, g, rect, wrap, form, joint=False)
        assert not did
        assert torch.equal(got, strips)
    x0, x1, y0, y1 = rect
    out = _core(got, g, w, th)
    mask = torch.ones(th, w, dtype=torch.bool, device=gpu)
    mask[y0:y1, x0:x1] = False
    assert bool((out[mask] == -3.0).all()) and bool((out[~mask] != -3.0).all())
    return g, src, out, th


@pytest.mark.parametrize("wrap", [True, False])
@pytest.mark.parametrize("h", HEIGHTS)
@pytest.mark.parametrize("w", WIDTHS)
def test_split_group_bitwise_sum_form(gpu, w, h, wrap):
    g, src, out, th = _check(gpu, w, h, wrap, "sum")
    if wrap and th == h:  # the whole torus: the CPU-order sum reference, as for the headline pass
        assert torch.equal(out, jacobi_sum_reference_global(_core(src, g, w, h).clone(), S))


@pytest.mark.parametrize("wrap", [True, False])
@pytest.mark.parametrize("form", ["step", "scaled"])
def test_split_group_bitwise_other_bodies(gpu, form, wrap):
    # The scaled body runs in the joint windows only (per step with them off): one oracle.
    _check(gpu, OWG + 224, 97, wrap, form, joint_oracle=form != "scaled")


@pytest.mark.parametrize("balanced", [True, False])
@pytest.mark.parametrize("wrap", [True, False])
def test_share_crosses_into_the_split_group(gpu, wrap, balanced):
    """Three groups x 600 rows on 4 workgroups (the grid of a GPU shared by 64
    processes): the linear space is 600 + 600 + 300 long, so the last workgroup's
    share starts in the second full group and ends in the split one."""
    H = hip()
    w, h, share = 2 * OWG + 224, 600, 64
    blocks = max(1, H.device_cu_count() // share)
    total = 2 * h + h // 2
    if balanced:  # fill: 59 row iterations per chunk of the 12 + 12 ascending pass (pipe_fill_rows)
        st = core().balanced_starts(3, h, blocks, 59, h // 2)
    else:
        st = [min(i * -(-total // blocks), total) for i in range(blocks + 1)]
    assert st[-1] == total and any(a < 2 * h < b for a, b in zip(st, st[1:])), st
    old = H.gpu_share(), H.pipe_balanced()
    try:
        H.set_gpu_share(share)
        H.set_pipe_balanced(balanced)
        _check(gpu, w, h, wrap, "sum")
    finally:
        H.set_gpu_share(old[0])
        H.set_pipe_balanced(old[1])
