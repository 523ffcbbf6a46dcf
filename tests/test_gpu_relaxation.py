"""Chebyshev relaxation on the GPU: the level-table kernels
(ops.stencil5_tb_levels, ops.stencil5_tb_held_levels) bit for bit against
ops.jacobi_held_levels_reference and against the uniform per-step kernels, and
the solver's cycle (call shapes, graphs, the torch backend, 2 x 2 ranks sharing
the GPU, checkpoint resume, the forms that ran, convergence, the range guard)."""
import os

import pytest
import torch

from cuda_mpi_scratch_amd import core, hip, ops
from cuda_mpi_scratch_amd.ops.stencil import dtype_name
from tests.relaxation_worker import BOUNDARY, launch, make

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
_CACHE = {}


def _geom(w, h, ring, dtype):
    return core().TileGeom.aligned(w, h, ring, ring, torch.tensor([], dtype=dtype).element_size())


def _full(buf, g):
    return buf.view(g.total_height(), g.pitch)[:, g.x_origin:g.x_origin + g.total_width()]


def _core(buf, g):
    return _full(buf, g)[g.halo_y:g.halo_y + g.height, g.halo_x:g.halo_x + g.width]


def _tile(gpu, w, h, S, dtype):
    """A tile whose core and ghost ring are random in [-1, 1] (padding zero),
    the cycle of its grid, and -- made once per shape -- nothing else."""
    key = (w, h, S, dtype)
    if key not in _CACHE:
        g = _geom(w, h, S, dtype)
        gen = torch.Generator(device="cpu").manual_seed(w + h + S)
        full = (torch.rand(g.total_height(), g.total_width(), generator=gen, dtype=torch.float64) * 2 - 1).to(dtype)
        src = torch.zeros(g.alloc_elems(), dtype=dtype, device=gpu)
        _full(src, g).copy_(full)
        t = core().chebyshev_cycle(w, h, 0.2, 0.2, S)
        _CACHE[key] = (g, full, src, t["center"], t["neighbor"])
    return _CACHE[key]


def _reference(w, h, S, dtype, hold):
    """The reference's core, once per (tile, hold) and left unchanged."""
    key = ("ref", w, h, S, dtype, hold)
    if key not in _CACHE:
        _, full, _, cen, nei = _CACHE[(w, h, S, dtype)]
        _CACHE[key] = ops.jacobi_held_levels_reference(full, cen, nei, hold, S)[S:S + h, S:S + w].contiguous()
    return _CACHE[key]


def _assert_bitwise(what, got, ref):
    diff = got != ref
    n = int(diff.sum())
    worst = (got.double() - ref.double()).abs().max().item() if n else 0.0
    print(f"{what}: {n} of {got.numel()} cells differ, max |diff| = {worst:.3e}")
    assert n == 0


def _assert_ring_untouched(dst, g):
    m = torch.ones(g.total_height(), g.total_width(), dtype=torch.bool)
    m[g.halo_y:g.halo_y + g.height, g.halo_x:g.halo_x + g.width] = False
    assert (_full(dst, g).cpu()[m] == -3.0).all(), "the kernel wrote outside the core"
    rows = dst.view(g.total_height(), g.pitch)
    assert (rows[:, :g.x_origin] == -3.0).all() and (rows[:, g.x_origin + g.total_width():] == -3.0).all()


# ------------------------------------------------------------------ kernels
# fp32: two column groups of the joint pipeline (912 / 904 columns), the second
# ragged, several row shares; fp64: 944 (8 + 8) and 4 x 232 columns per group.
@pytest.mark.parametrize("w,h,S,dtype", [(1040, 160, 20, F32), (1040, 160, 24, F32), (1008, 96, 12, F64),
                                         (1008, 96, 16, F64)])
def test_pipeline_levels_match_reference_bitwise(gpu, w, h, S, dtype):
    g, _, src, cen, nei = _tile(gpu, w, h, S, dtype)
    dst = torch.full_like(src, -3.0)
    ops.stencil5_tb_levels(src, dst, g, 0, w, 0, h, cen, nei)
    assert hip().last_stencil_dispatch() == "stream_pipe_levels"
    torch.cuda.synchronize()
    _assert_bitwise(f"pipeline levels {w}x{h} S={S} {dtype_name(src)}", _core(dst, g).cpu(), _reference(w, h, S, dtype, 0))
    _assert_ring_untouched(dst, g)


@pytest.mark.parametrize("hold", range(16))
@pytest.mark.parametrize("S,dtype", [(20, F32), (16, F64)])
def test_held_levels_match_reference_bitwise(gpu, S, dtype, hold):
    w, h = 72, 40
    g, _, src, cen, nei = _tile(gpu, w, h, S, dtype)
    dst = torch.full_like(src, -3.0)
    ops.stencil5_tb_held_levels(src, dst, g, 0, w, 0, h, cen, nei, hold)
    assert hip().last_stencil_dispatch() == "held_levels"
    torch.cuda.synchronize()
    _assert_bitwise(f"held levels S={S} {dtype_name(src)} hold={hold}", _core(dst, g).cpu(), _reference(w, h, S, dtype, hold))
    _assert_ring_untouched(dst, g)


# One tall narrow and one wide flat frame strip, S wide: the tile shapes the
# solver's frame takes.
@pytest.mark.parametrize("rect", [(0, 20, 20, 180), (0, 264, 0, 20)])
def test_held_levels_frame_strips(gpu, rect):
    w, h, S, hold = 264, 200, 20, 15
    x0, x1, y0, y1 = rect
    g, _, src, cen, nei = _tile(gpu, w, h, S, F32)
    dst = torch.full_like(src, -3.0)
    ops.stencil5_tb_held_levels(src, dst, g, x0, x1, y0, y1, cen, nei, hold)
    torch.cuda.synchronize()
    got, ref = _core(dst, g).cpu(), _reference(w, h, S, F32, hold)
    _assert_bitwise(f"frame strip {rect}", got[y0:y1, x0:x1], ref[y0:y1, x0:x1])
    outside = torch.ones(h, w, dtype=torch.bool)
    outside[y0:y1, x0:x1] = False
    assert (got[outside] == -3.0).all(), "cells outside the rectangle were written"
    _assert_ring_untouched(dst, g)


@pytest.mark.parametrize("w,h,S,dtype", [(1040, 160, 20, F32), (1040, 160, 24, F32), (1008, 96, 12, F64),
                                         (1008, 96, 16, F64)])
def test_uniform_table_reproduces_the_per_step_kernels(gpu, w, h, S, dtype):
    g, _, src, _, _ = _tile(gpu, w, h, S, dtype)
    c0, c1 = 0.5, 0.125
    s = torch.cuda.current_stream().cuda_stream
    a, b = torch.full_like(src, -3.0), torch.full_like(src, -3.0)
    ops.stencil5_tb_levels(src, a, g, 0, w, 0, h, [c0] * S, [c1] * S)
    hip().stencil5_tb(src.data_ptr(), b.data_ptr(), g, S, 0, w, 0, h, c0, c1, False, dtype_name(src), s, "auto", False,
                      -1.0)
    assert hip().last_stencil_dispatch() == "stream_pipe"
    torch.cuda.synchronize()
    assert torch.equal(a, b), "a uniform level table differs from the per-step stencil5_tb"
    for hold in (0, 15, 6):
        a.fill_(-3.0)
        b.fill_(-3.0)
        ops.stencil5_tb_held_levels(src, a, g, 0, w, 0, h, [c0] * S, [c1] * S, hold)
        ops.stencil5_tb_held(src, b, g, S, 0, w, 0, h, c0, c1, hold)
        torch.cuda.synchronize()
        assert torch.equal(a, b), f"a uniform level table differs from the per-step stencil5_tb_held (hold {hold})"


# The held tile is one body for its three coefficient sources (uniform pair,
# level table, level table + correction tile). Widths that are no whole number
# of vectors (70 fp32, 35 fp64) put a ragged last vector beside the held right
# side; the three rectangles take the general, the narrow and the flat tile.
@pytest.mark.parametrize("shape", ["general", "narrow", "flat"])
@pytest.mark.parametrize("w,S,dtype", [(70, 20, F32), (35, 12, F64)])
def test_held_tile_is_one_body_for_its_three_sources(gpu, w, S, dtype, shape):
    h, c0, c1 = 40, 0.5, 0.125
    g, _, src, _, _ = _tile(gpu, w, h, S, dtype)
    N = 16 // src.element_size()
    x0, x1, y0, y1 = {"general": (0, w, 0, h), "narrow": (0, N * ((S + N - 1) // N), 0, h), "flat": (0, w, 0, S)}[shape]
    gen = torch.Generator(device="cpu").manual_seed(7 * w + S)
    corr = (torch.rand(g.alloc_elems(), generator=gen, dtype=torch.float64) * 2 - 1).to(dtype).to(gpu)
    for hold in (0, 15, ops.HOLD_RIGHT):
        uni, lev, got = (torch.full_like(src, -3.0) for _ in range(3))
        ops.stencil5_tb_held(src, uni, g, S, x0, x1, y0, y1, c0, c1, hold)
        assert hip().last_stencil_dispatch() == "tb_held"
        ops.stencil5_tb_held_levels(src, lev, g, x0, x1, y0, y1, [c0] * S, [c1] * S, hold)
        assert hip().last_stencil_dispatch() == "held_levels"
        ops.stencil5_tb_held_levels(src, got, g, x0, x1, y0, y1, [c0] * S, [c1] * S, hold, corr=corr)
        assert hip().last_stencil_dispatch() == "held_levels_src"
        torch.cuda.synchronize()
        assert torch.equal(uni, lev), f"{shape} hold {hold}: the uniform table differs from stencil5_tb_held"
        want = lev.clone()
        _core(want, g)[y0:y1, x0:x1] += _core(corr, g)[y0:y1, x0:x1]  # one rounded add in the element type
        assert torch.equal(got, want), f"{shape} hold {hold}: with corr, not the pass plus corr on the rectangle"
        outside = torch.ones(g.alloc_elems(), dtype=torch.bool, device=gpu)
        _core(outside, g)[y0:y1, x0:x1] = False
        assert (got[outside] == -3.0).all() and (_core(got, g)[y0:y1, x0:x1] != -3.0).all()


def test_level_depths_without_kernels_are_errors(gpu):
    g, _, src, _, _ = _tile(gpu, 72, 40, 20, F32)
    dst = torch.empty_like(src)
    with pytest.raises(Exception, match="has no kernel"):
        ops.stencil5_tb_levels(src, dst, g, 0, 72, 0, 40, [0.2] * 16, [0.2] * 16)
    with pytest.raises(Exception, match="has no kernel"):
        ops.stencil5_tb_held_levels(src, dst, g, 0, 72, 0, 40, [0.2] * 12, [0.2] * 12, 15)


# ------------------------------------------------------------------- solver
SOLVER = {"w": 1040, "h": 160, "dtype": "f32", "time_block": 20, "seed": 11}


def _field(st):
    st.synchronize()
    return st.core_view().cpu().clone()


@pytest.fixture(scope="module")
def one_rank_60(gpu):
    st = make(SOLVER)
    st.run(60)
    return st, _field(st)


def test_solver_call_shapes_graphs_and_torch_backend_agree_bitwise(gpu, one_rank_60):
    st, ref = one_rank_60
    assert st.time_block == 20 and st.cycle == 20
    split = make(SOLVER)
    for _ in range(3):
        split.run(20)
    assert torch.equal(_field(split), ref), "run(60) differs from three run(20)"
    eager = make(dict(SOLVER, graph=False))
    eager.run(60)
    assert torch.equal(_field(eager), ref), "graph=False differs from the graph replay"
    assert st.solver.graph_active() and not eager.solver.graph_active(), (st.graph_status(), eager.graph_status())
    # The forms that ran (eager: the frame strips are the pass's last launches).
    assert hip().last_stencil_dispatch() == "held_levels"
    note = st.relaxation_note()
    print(note, "|", st.solver.sum_form_note(), "|", st.fixed_edge_note())
    assert "M = 20" in note and "growth" in note and "level passes" in note
    assert "per-step" in st.solver.sum_form_note() and not st.sum_form_active
    assert st.solver.relaxation_info()["active"]
    with pytest.raises(Exception, match="multiple of the cycle length 20"):
        st.run(30)
    # The torch backend on the same device: one level per iteration through ops.stencil5.
    torch_be = make(dict(SOLVER, backend="torch"))
    assert torch_be.solver is None and torch_be.cycle == 20
    torch_be.run(60)
    assert torch.equal(_field(torch_be), ref), "the native cycle differs from the torch backend's"


def test_solver_interior_runs_the_level_pipeline(gpu):
    st = make(dict(SOLVER, graph=False))
    sp = core().fixed_edge_split(1040, 160, 20, 4, 15)
    x0, x1, y0, y1 = sp["interior"]
    assert (x1 - x0) % 4 == 0 and x1 - x0 > 912  # two column groups
    t = st.solver.relaxation_info()
    dst = torch.empty_like(st.a)
    ops.stencil5_tb_levels(st.a, dst, st.geom, x0, x1, y0, y1, t["center"], t["neighbor"])
    assert hip().last_stencil_dispatch() == "stream_pipe_levels"
    torch.cuda.synchronize()


def test_solver_2x2_ranks_equal_one_rank_bitwise(gpu, one_rank_60):
    _, ref = one_rank_60
    four = launch(4, dict(SOLVER, dims="2x2", runs=[60]))
    assert all(r["time_block"] == 20 and r["cycle"] == 20 and "level passes" in r["note"] for r in four), four
    assert four[0]["grid"] == ref.contiguous().numpy().tobytes().hex()


def test_solver_resume_continues_bitwise(gpu, tmp_path):
    path = os.path.join(tmp_path, "cycle40.grid")
    a = make(SOLVER)
    a.run(40)
    a.synchronize()
    a.save_checkpoint(path)
    a.run(40)
    b = make(SOLVER)
    hdr = b.load_checkpoint(path)
    assert hdr.iteration == 40
    b.run(40)
    assert a.iteration == b.iteration == 80
    assert torch.equal(_field(a), _field(b)), "a resumed run differs from the uninterrupted one"


def _reference_iterations(w, h, M, tol, cap):
    """Iterations the cycle needs in a float64 CPU reference (zero start, the
    fixed edges BOUNDARY, linf residual of the base operator checked at cycle ends)."""
    t = core().chebyshev_cycle(w, h, 0.2, 0.2, M)
    p = torch.zeros(h + 2, w + 2, dtype=torch.float64)
    p[0, 1:-1], p[-1, 1:-1], p[1:-1, 0], p[1:-1, -1] = (BOUNDARY[k] for k in ("top", "bottom", "left", "right"))
    its = 0
    while its < cap:
        for c0, c1 in zip(t["center"], t["neighbor"]):
            p[1:-1, 1:-1] = c1 * ((p[:-2, 1:-1] + p[2:, 1:-1]) + (p[1:-1, :-2] + p[1:-1, 2:])) + c0 * p[1:-1, 1:-1]
        its += M
        if ops.residual5_reference(p, 1, 0.2, 0.2)[0] <= tol:
            return its
    raise AssertionError(f"the reference cycle did not reach {tol} in {cap} iterations")


def test_convergence_on_the_device(gpu):
    args = {"w": 256, "h": 192, "dtype": "f64", "time_block": 16, "zero": True}
    ref_its = _reference_iterations(256, 192, 16, 1e-6, 40000)
    max_iters = 2 * ref_its
    st = make(args)
    out = st.run_until(1e-6, max_iters)
    print(f"reference {ref_its} iterations; chebyshev {out['iterations']} (residual {out['residual']:.3e}, "
          f"check_every {out['check_every']}); {st.relaxation_note()}")
    assert out["converged"], out
    assert out["iterations"] <= max_iters and out["iterations"] % 16 == 0
    plain = make(dict(args, relaxation="none"))
    res = plain.run_until(1e-6, 5 * max_iters)
    print(f"plain Jacobi: {res['iterations']} iterations, residual {res['residual']:.3e}, converged {res['converged']}")
    assert not res["converged"]
    assert res["iterations"] >= 5 * out["iterations"]


def test_range_guard_runs_the_plain_pass(gpu):
    st = make({"w": 264, "h": 200, "dtype": "f32", "time_block": 20, "graph": False})
    growth = st.solver.relaxation_info()["growth"]
    big = 1.0e36
    assert growth * big >= torch.finfo(torch.float32).max / 4
    st.set_boundary(top=big)
    st.run(20)
    field = _field(st)
    note = st.relaxation_note()
    print(note)
    assert "plain per-step passes" in note and "range guard" in note
    assert not st.solver.relaxation_info()["active"]
    assert hip().last_stencil_dispatch() == "tb_held"
    assert torch.isfinite(field).all()
    # Back inside the range the level passes return.
    st.synchronize()
    st.a.zero_()
    st.b.zero_()
    st.set_boundary(**BOUNDARY)
    st.run(20)
    st.synchronize()
    assert "level passes" in st.relaxation_note() and hip().last_stencil_dispatch() == "held_levels"
