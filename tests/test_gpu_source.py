"""The source term (u' = A u + g) on the GPU: the level-table kernels with a
correction tile (ops.stencil5_tb_levels / stencil5_tb_held_levels, corr=) bit
for bit against the same launch without it plus a torch add, what they may read
and write, the residual kernel with a source, the native build of the
correction, and the solver (call shapes, graphs, the torch backend, 2 x 2 ranks
sharing the GPU, accuracy against the per-step definition, checkpoint resume, a
manufactured Poisson solution, the range guard)."""
import math
import os

import numpy as np
import pytest
import torch

from cuda_mpi_scratch_amd import core, hip, ops
from cuda_mpi_scratch_amd.ops.relaxation import _fma
from cuda_mpi_scratch_amd.ops.stencil import dtype_name
from tests.source_worker import global_source, launch, make
from tests.test_source_cpu import C0, C1, manufactured

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
    """Per shape, made once and left unchanged: a tile whose core and ghost ring
    are random in [-1, 1] (padding zero), the Chebyshev cycle of its grid, and a
    correction tile whose core is random in [-1, 1] and whose ghost ring and
    padding are NaN."""
    key = (w, h, S, dtype)
    if key not in _CACHE:
        g = _geom(w, h, S, dtype)
        gen = torch.Generator(device="cpu").manual_seed(w + h + S)
        full = (torch.rand(g.total_height(), g.total_width(), generator=gen, dtype=torch.float64) * 2 - 1).to(dtype)
        src = torch.zeros(g.alloc_elems(), dtype=dtype, device=gpu)
        _full(src, g).copy_(full)
        corr = torch.full((g.alloc_elems(),), float("nan"), dtype=dtype, device=gpu)
        _core(corr, g).copy_((torch.rand(h, w, generator=gen, dtype=torch.float64) * 2 - 1).to(dtype))
        t = core().chebyshev_cycle(w, h, 0.2, 0.2, S)
        _CACHE[key] = (g, src, corr, t["center"], t["neighbor"])
    return _CACHE[key]


def _assert_ring_untouched(dst, g):
    m = torch.ones(g.total_height(), g.total_width(), dtype=torch.bool)
    m[g.halo_y:g.halo_y + g.height, g.halo_x:g.halo_x + g.width] = False
    assert (_full(dst, g).cpu()[m] == -3.0).all(), "the kernel wrote outside the core"
    rows = dst.view(g.total_height(), g.pitch)
    assert (rows[:, :g.x_origin] == -3.0).all() and (rows[:, g.x_origin + g.total_width():] == -3.0).all()


def _assert_rect_is_pass_plus_corr(what, got, plain, corr, g, rect):
    """Inside the rectangle: bitwise the pass without corr plus a torch add of
    corr's cells on the device; outside it: the -3.0 sentinel."""
    x0, x1, y0, y1 = rect
    want = _core(plain, g)[y0:y1, x0:x1] + _core(corr, g)[y0:y1, x0:x1]
    have = _core(got, g)[y0:y1, x0:x1]
    n = int((have != want).sum())
    print(f"{what}: {n} of {have.numel()} cells differ from pass + corr")
    assert torch.isfinite(have).all(), "NaN from corr's ring or padding reached a stored cell"
    assert n == 0
    outside = torch.ones(g.height, g.width, dtype=torch.bool, device=got.device)
    outside[y0:y1, x0:x1] = False
    assert (_core(got, g)[outside] == -3.0).all(), "cells outside the rectangle were written"
    _assert_ring_untouched(got, g)


# ------------------------------------------------------------------ kernels
# The shapes of test_pipeline_levels_match_reference_bitwise (two column groups,
# the second ragged, several row shares; at S = 24 the 136 columns left for the
# second group make it a split narrow group), then the edges of the split at
# S = 24 (tests/test_gpu_pipe_split.py): 904 + 440 columns (split), 904 + 444
# (not split) and a single narrow group.
PIPE = [(1040, 160, 20, F32, False), (1040, 160, 24, F32, True), (1008, 96, 12, F64, False),
        (1008, 96, 16, F64, False), (904 + 440, 97, 24, F32, True), (904 + 444, 97, 24, F32, False),
        (224, 40, 24, F32, True)]


@pytest.mark.parametrize("w,h,S,dtype,split", PIPE)
def test_pipeline_with_corr_is_the_pass_plus_corr_bitwise(gpu, w, h, S, dtype, split):
    g, src, corr, cen, nei = _tile(gpu, w, h, S, dtype)
    plain, got = torch.full_like(src, -3.0), torch.full_like(src, -3.0)
    ops.stencil5_tb_levels(src, plain, g, 0, w, 0, h, cen, nei)
    assert hip().last_stencil_dispatch() == "stream_pipe_levels"
    ops.stencil5_tb_levels(src, got, g, 0, w, 0, h, cen, nei, corr=corr)
    assert hip().last_stencil_dispatch() == "stream_pipe_levels_src"
    assert hip().last_pipe_split() == split
    torch.cuda.synchronize()
    _assert_rect_is_pass_plus_corr(f"pipeline + corr {w}x{h} S={S} {dtype_name(src)}", got, plain, corr, g, (0, w, 0, h))
    again = torch.full_like(src, -3.0)
    ops.stencil5_tb_levels(src, again, g, 0, w, 0, h, cen, nei, corr=None)  # None: exactly the launch without it
    assert hip().last_stencil_dispatch() == "stream_pipe_levels"
    torch.cuda.synchronize()
    assert torch.equal(again, plain)


@pytest.mark.parametrize("hold", [0, 6, 15])
@pytest.mark.parametrize("S,dtype", [(20, F32), (16, F64)])
@pytest.mark.parametrize("x1", [72, 70])  # 70: not a whole number of vectors
def test_held_with_corr_is_the_pass_plus_corr_bitwise(gpu, S, dtype, hold, x1):
    w, h = 72, 40
    g, src, corr, cen, nei = _tile(gpu, w, h, S, dtype)
    plain, got = torch.full_like(src, -3.0), torch.full_like(src, -3.0)
    ops.stencil5_tb_held_levels(src, plain, g, 0, x1, 0, h, cen, nei, hold)
    assert hip().last_stencil_dispatch() == "held_levels"
    ops.stencil5_tb_held_levels(src, got, g, 0, x1, 0, h, cen, nei, hold, corr=corr)
    assert hip().last_stencil_dispatch() == "held_levels_src"
    torch.cuda.synchronize()
    _assert_rect_is_pass_plus_corr(f"held + corr S={S} {dtype_name(src)} hold={hold} x1={x1}", got, plain, corr, g,
                                   (0, x1, 0, h))


@pytest.mark.parametrize("rect", [(0, 20, 20, 180), (0, 264, 0, 20)])
def test_held_frame_strips_with_corr(gpu, rect):
    w, h, S, hold = 264, 200, 20, 15
    x0, x1, y0, y1 = rect
    g, src, corr, cen, nei = _tile(gpu, w, h, S, F32)
    plain, got = torch.full_like(src, -3.0), torch.full_like(src, -3.0)
    ops.stencil5_tb_held_levels(src, plain, g, x0, x1, y0, y1, cen, nei, hold)
    ops.stencil5_tb_held_levels(src, got, g, x0, x1, y0, y1, cen, nei, hold, corr=corr)
    assert hip().last_stencil_dispatch() == "held_levels_src"
    torch.cuda.synchronize()
    _assert_rect_is_pass_plus_corr(f"frame strip + corr {rect}", got, plain, corr, g, rect)


def test_thin_rectangle_with_corr_falls_back_to_the_held_tile(gpu):
    w, h, S = 72, 40, 20
    g, src, corr, cen, nei = _tile(gpu, w, h, S, F32)
    plain, got = torch.full_like(src, -3.0), torch.full_like(src, -3.0)
    ops.stencil5_tb_levels(src, plain, g, 0, 24, 0, h, cen, nei)
    ops.stencil5_tb_levels(src, got, g, 0, 24, 0, h, cen, nei, corr=corr)
    assert hip().last_stencil_dispatch() == "held_levels_src"
    torch.cuda.synchronize()
    _assert_rect_is_pass_plus_corr("thin rectangle + corr", got, plain, corr, g, (0, 24, 0, h))


# ------------------------------------------------- residual with a source
TOL = {F32: 2e-6, F64: 1e-14}  # the project's TOL, as in tests/test_gpu_residual.py


def _bits(x):
    return torch.tensor(x, dtype=torch.float64).view(torch.int64).item()


@pytest.mark.parametrize("dtype", [F32, F64])
def test_residual_with_a_source(gpu, dtype):
    w, h, ring = 264, 200, 12
    g = _geom(w, h, ring, dtype)
    gen = torch.Generator(device="cpu").manual_seed(5)
    full = torch.rand(g.total_height(), g.total_width(), generator=gen, dtype=torch.float64).to(dtype)
    gcore = ((torch.rand(h, w, generator=gen, dtype=torch.float64) * 2 - 1) * 0.01).to(dtype)
    src = torch.zeros(g.alloc_elems(), dtype=dtype, device=gpu)
    _full(src, g).copy_(full)
    gt = torch.full((g.alloc_elems(),), float("nan"), dtype=dtype, device=gpu)  # NaN ring and padding
    _core(gt, g).copy_(gcore)
    linf, sumsq = ops.stencil5_residual(src, g, C0, C1, source=gt)
    assert math.isfinite(linf) and math.isfinite(sumsq)
    assert (_bits(linf), _bits(sumsq)) == tuple(map(_bits, ops.stencil5_residual(src, g, C0, C1, source=gt)))
    # The kernel's own operations on the CPU, a correctly rounded fma: linf bit for bit.
    c = full[ring:ring + h, ring:ring + w]
    sums = (full[ring - 1:ring - 1 + h, ring:ring + w] + full[ring + 1:ring + 1 + h, ring:ring + w]) + \
        (full[ring:ring + h, ring - 1:ring - 1 + w] + full[ring:ring + h, ring + 1:ring + 1 + w])
    step = _fma(C1, sums.contiguous(), (torch.tensor(C0, dtype=dtype) * c).contiguous())
    r = ((step + gcore) - c).double()
    l2 = math.sqrt(sumsq)
    rl, r2 = ops.residual5_reference(full, ring, C0, C1, source=gcore)
    print(f"residual + source {NAME(dtype)}: linf {linf:.9g} (exact fma {float(r.abs().max()):.9g}, reference {rl:.9g}), "
          f"l2 {l2:.9g} (reference {r2:.9g})")
    assert linf == float(r.abs().max())
    assert abs(linf - rl) <= 2 * TOL[dtype]
    assert abs(l2 - r2) <= 2 * TOL[dtype] * math.sqrt(w * h)
    assert abs(l2 - math.sqrt(float((r * r).sum()))) <= 1e-12 * l2
    assert linf != ops.stencil5_residual(src, g, C0, C1)[0]  # the source matters


def NAME(dtype):
    return "f32" if dtype == F32 else "f64"


# ------------------------------------------------------------------ the build
@pytest.mark.parametrize("relaxation", ["chebyshev", "none"])
@pytest.mark.parametrize("dtype,M", [("f32", 20), ("f64", 16)])
def test_native_correction_equals_the_reference_bitwise(gpu, dtype, M, relaxation):
    args = {"w": 264, "h": 200, "dtype": dtype, "time_block": M, "relaxation": relaxation}
    st = make(args)
    assert st.solver is not None and st.source_correction() is None
    g = global_source(args)
    st.set_source(g)
    t = st.solver.relaxation_info()
    assert t["cycle"] == M
    want = ops.source_correction_reference(g.to(st.device), t["center"], t["neighbor"], C1, st.dtype)
    got = st.source_correction()
    n = int((got != want).sum())
    print(f"native G {dtype} M={M} {relaxation}: {n} of {got.numel()} cells differ, max |G| {float(got.abs().max()):.3e}")
    assert n == 0 and bool(got.any())
    st.set_source(None)
    assert st.source_correction() is None and not st.solver.source_set()


# ------------------------------------------------------------------- solver
BIG = [{"w": 1040, "h": 200, "dtype": "f32", "time_block": 24, "seed": 11},
       {"w": 1008, "h": 160, "dtype": "f64", "time_block": 16, "seed": 11}]


def _field(st):
    st.synchronize()
    return st.core_view().cpu().clone()


def _run(args, runs, g="default", **kw):
    st = make(dict(args, **kw))
    start = st.full_view().cpu().clone()
    st.set_source(global_source(args) if isinstance(g, str) else g)
    for n in runs:
        st.run(n)
    return st, _field(st), start


@pytest.fixture(scope="module", params=BIG, ids=["f32-M24", "f64-M16"])
def one_rank(gpu, request):
    args = request.param
    st, field, start = _run(args, [3 * args["time_block"]])
    return args, st, field, start


def test_solver_call_shapes_graphs_and_torch_backend_agree_bitwise(gpu, one_rank):
    args, st, ref, _ = one_rank
    M = args["time_block"]
    assert st.time_block == M and st.cycle == M and st.solver.source_set()
    assert torch.equal(_run(args, [M] * 3)[1], ref), "run(3M) differs from three run(M)"
    eager, field, _ = _run(args, [3 * M], graph=False)
    assert torch.equal(field, ref), "graph=False differs from the graph replay"
    assert st.solver.graph_active() and not eager.solver.graph_active(), (st.graph_status(), eager.graph_status())
    assert hip().last_stencil_dispatch() == "held_levels_src"  # eager: the frame strips are the pass's last launches
    note = st.relaxation_note()
    print(note, "|", st.solver.sum_form_note(), "|", st.fixed_edge_note())
    assert "source" in note and "per-step" in st.solver.sum_form_note() and "source" in st.solver.sum_form_note()
    assert "4 frame strips" in st.fixed_edge_note()
    with pytest.raises(Exception, match=f"multiple of the cycle length {M}"):
        st.run(M + 1)
    tb, field, _ = _run(args, [3 * M], backend="torch")
    assert tb.solver is None and tb.cycle == M
    assert torch.equal(field, ref), "the native cycle with a source differs from the torch backend's"
    # The interior of the pass: the pipeline with the correction.
    sp = core().fixed_edge_split(args["w"], args["h"], M, 4, 15)
    x0, x1, y0, y1 = sp["interior"]
    t = st.solver.relaxation_info()
    corr = torch.zeros_like(st.a)
    ops.stencil5_tb_levels(st.a, torch.empty_like(st.a), st.geom, x0, x1, y0, y1, t["center"], t["neighbor"], corr=corr)
    assert hip().last_stencil_dispatch() == "stream_pipe_levels_src"
    torch.cuda.synchronize()


def test_clearing_the_source_returns_to_the_homogeneous_kernels(gpu, one_rank):
    args, _, ref, _ = one_rank
    M = args["time_block"]
    g = global_source(args)
    # From the start: set, clear, run.
    cleared = make(dict(args, graph=False))
    cleared.set_source(g)
    cleared.set_source(None)
    cleared.run(3 * M)
    cleared.synchronize()
    assert hip().last_stencil_dispatch() == "held_levels"
    base = make(args, source=False)  # the solver without a source term: the kernels as they were
    base.run(3 * M)
    want = _field(base)
    assert torch.equal(_field(cleared), want), "set_source(None) does not give the homogeneous run back"
    assert not torch.equal(want, ref)
    assert torch.equal(_run(args, [3 * M], g=0.0)[1], want)  # G is exactly 0
    # After a cycle with the source: clear, then one homogeneous cycle from that field.
    x = _run(args, [M], graph=False)[0]
    x.synchronize()
    snap = x.current().clone()
    x.set_source(None)
    x.run(M)
    x.synchronize()
    assert hip().last_stencil_dispatch() == "held_levels"
    y = make(dict(args, graph=False), source=False)
    y.current().copy_(snap)
    y.field_changed()
    y.run(M)
    assert torch.equal(_field(x), _field(y))


def test_uniform_table_with_a_source_and_without_equals_plain_jacobi(gpu):
    args = dict(BIG[0], relaxation="none")
    M = args["time_block"]
    st, with_zero, _ = _run(args, [2 * M], g=None)
    assert "uniform level table" in st.relaxation_note() and st.cycle == M
    plain = make(args, source=False)
    plain.run(2 * M)
    assert torch.equal(with_zero, _field(plain)), "the uniform level table differs from the plain per-step passes"
    tb = _run(args, [2 * M], backend="torch")[1]
    assert torch.equal(_run(args, [2 * M])[1], tb)


@pytest.mark.parametrize("dtype,M", [("f32", 20), ("f64", 16)])
def test_solver_2x2_ranks_equal_one_rank_bitwise(gpu, dtype, M):
    args = {"w": 120, "h": 80, "dtype": dtype, "time_block": M, "runs": [M], "tol": 0.0, "max_iters": 2 * M,
            "check_every": M, "norm": "l2"}
    st = make(args)
    st.set_source(global_source(args))
    st.run(M)
    one = st.run_until(0.0, 2 * M, M, "l2")
    ref = _field(st)
    four = launch(4, dict(args, dims="2x2", backend="ipc"))
    assert all(r["time_block"] == M and r["cycle"] == M and r["iteration"] == 3 * M for r in four), four
    assert four[0]["grid"] == ref.contiguous().numpy().tobytes().hex()
    assert all(r["until"] == four[0]["until"] for r in four)
    h4, h1 = four[0]["until"]["history"], one["history"]
    assert [x[0] for x in h4] == [x[0] for x in h1] == [0, M, 2 * M]
    assert [x[1] for x in h4] == [x[1] for x in h1]  # linf: a max, order-free
    assert all(abs(a[2] - b[2]) <= 1e-12 * b[2] for a, b in zip(h4, h1))  # l2: per-tile partial sums


def test_accuracy_against_the_per_step_definition(gpu, one_rank):
    """The native result under the 4 err_step rule of the CPU algebra test."""
    args, st, got, start = one_rank
    M, w, h = args["time_block"], args["w"], args["h"]
    hy, hx = st.geom.halo_y, st.geom.halo_x
    full = start[hy - 1:hy + h + 1, hx - 1:hx + w + 1].contiguous()
    g = global_source(args)
    t = st.solver.relaxation_info()
    exact = ops.jacobi_source_per_step_reference(full, g, t["center"], t["neighbor"], C1, 15, 3, dtype=np.longdouble)
    step = ops.jacobi_source_per_step_reference(full, g, t["center"], t["neighbor"], C1, 15, 3)
    to_ld = lambda x: x.double().numpy().astype(np.longdouble)  # noqa: E731
    err_step = float(np.abs(to_ld(step) - exact).max())
    err_corr = float(np.abs(to_ld(got) - exact[1:-1, 1:-1]).max())
    print(f"{w}x{h} {args['dtype']} M={M}: err_step {err_step:.3e}, native err_corr {err_corr:.3e}, "
          f"ratio {err_corr / err_step:.3f}")
    assert err_step > 0 and err_corr <= 4 * err_step


def test_resume_continues_bitwise_after_set_source(gpu, tmp_path):
    args = BIG[0]
    M = args["time_block"]
    path = os.path.join(tmp_path, "source.grid")
    a = make(args)
    a.set_source(global_source(args))
    a.run(2 * M)
    a.synchronize()
    a.save_checkpoint(path)
    a.run(2 * M)
    b = make(args)
    hdr = b.load_checkpoint(path)
    assert hdr.iteration == 2 * M
    b.set_source(global_source(args))  # the source is not part of the checkpoint
    b.run(2 * M)
    assert a.iteration == b.iteration == 4 * M
    assert torch.equal(_field(a), _field(b)), "a resumed run differs from the uninterrupted one"


def test_manufactured_poisson_solution_on_the_device(gpu):
    w, h, M = 96, 64, 16
    u_star, g, a = manufactured(w, h)
    st = make({"w": w, "h": h, "dtype": "f64", "time_block": M, "zero": True, "boundary": "zero"})
    assert st.solver is not None
    st.set_source(g)
    out = st.run_until(1e-8, M * 200, norm="l2")
    err = float(torch.linalg.vector_norm(_field(st) - u_star))
    print(f"manufactured {w}x{h} on the device: {out['iterations']} iterations, l2 residual {out['residual']:.3e}, "
          f"||u - u*||_2 {err:.3e}, bound {1e-8 / a:.3e}")
    assert out["converged"], out["reason"]
    assert out["iterations"] <= M * 200 and out["iterations"] % M == 0
    assert err <= (1e-8 / a) * (1 + 1e-6)


def test_range_guard_with_a_source_is_an_error(gpu):
    st = make({"w": 264, "h": 200, "dtype": "f32", "time_block": 20, "graph": False})
    st.set_source(0.001)
    big = 1.0e36
    assert st.solver.relaxation_info()["growth"] * big >= torch.finfo(torch.float32).max / 4
    st.set_boundary(top=big)
    with pytest.raises(Exception, match="range guard"):
        st.run(20)


# --------------------------------------------------------------- CLI, app
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "build", "bin")


def test_cli_source(gpu):
    import json
    import subprocess
    import sys

    cmd = [sys.executable, "-m", "cuda_mpi_scratch_amd.models.stencil2d", "--global", "96x64", "--dtype", "f64",
           "--relaxation", "chebyshev", "--source", "1e-4", "--tol", "1e-9", "--max-iters", "3200", "--warmup", "0",
           "--no-sum-form", "--seed", "5"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=240, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    rec = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert rec["source"] == 1e-4 and rec["time_block"] == 16 and rec["backend"] == "local"
    from cuda_mpi_scratch_amd.models.stencil2d import Stencil2D, StencilConfig

    st = Stencil2D(StencilConfig(global_width=96, global_height=64, dims="1x1", dtype="f64", periodic=False,
                                 block_fixed_edges=True, relaxation="chebyshev", source=True, sum_form=False, seed=5))
    st.set_source(1e-4)
    want = st.run_until(1e-9, 3200)
    assert want["converged"] and want["iterations"] > 0
    assert rec["converged"] is True and rec["iterations"] == want["iterations"] and rec["residual"] == want["residual"]


def _mpiexec():
    import shutil

    return shutil.which("mpiexec", path="/opt/conda/bin") or shutil.which("mpiexec")


@pytest.mark.skipif(not (_mpiexec() and os.path.exists(os.path.join(BIN, "stencil2d"))), reason="MPI GPU apps not built")
def test_app_source(gpu, tmp_path):
    """--source on one rank (local) and on four ranks sharing the GPU (ipc): the
    same iterations and the same linf residual; without it another run."""
    import json
    import re
    import subprocess

    args = ["--global", "96x64", "--dtype", "f64", "--relaxation", "chebyshev", "--tol", "1e-9", "--iters", "3200",
            "--warmup", "0"]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    found = []
    for n, extra in ((1, ["--source", "1e-4"]), (4, ["--source", "1e-4"]), (1, ["--non-periodic", "--block-fixed-edges"])):
        r = subprocess.run([_mpiexec(), "-n", str(n), os.path.join(BIN, "stencil2d"), *args, *extra],
                           capture_output=True, text=True, timeout=240, cwd=tmp_path, env=env)
        assert r.returncode == 0, r.stderr[-3000:]
        m = re.search(r"^converged after (\d+) iterations, residual ([0-9.eE+-]+) \(linf\)$", r.stdout, re.M)
        assert m, r.stdout[-2000:]
        rec = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
        assert rec["converged"] is True and rec["iterations"] % 16 == 0
        assert rec["source"] == (1e-4 if "--source" in extra else None)
        found.append((int(m.group(1)), m.group(2)))
    assert found[0] == found[1]
    assert found[0] != found[2]
