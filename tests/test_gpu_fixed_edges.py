"""Time blocking beside fixed (non-periodic) edges: the held-side kernel
(ops.stencil5_tb_held) against its reference and against single steps, and the
solver's interior + frame pass (StencilConfig.block_fixed_edges) against the
one-exchange-per-iteration path it replaces, on one rank and on several ranks
sharing the GPU."""
import json
import os
import socket
import subprocess
import sys

import pytest
import torch

from cuda_mpi_scratch_amd import core, hip, ops
from cuda_mpi_scratch_amd.models.stencil2d import Stencil2D, StencilConfig
from cuda_mpi_scratch_amd.ops.stencil import dtype_name

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
F32, F64 = torch.float32, torch.float64
TOL = {F32: 2e-6, F64: 1e-14}  # the project's tolerances (test_gpu_headline.py)

KERNEL_CASES = [
    (264, 200, 12, F32, 15),
    (262, 200, 5, F32, 15),    # ragged right edge, x apron (8) wider than S
    (40, 24, 12, F32, 15),     # tile smaller than the apron
    (264, 300, 20, F32, 5),    # top and left held, bottom and right advance as cells
    (264, 200, 32, F32, 10),   # bottom and right held, deepest block
    (200, 136, 16, F64, 15),
    (202, 136, 7, F64, 9),     # top and right held, ragged fp64 width
    (264, 200, 12, F32, 12),   # left and right held only (rows periodic, columns fixed)
]


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _geom(w, h, ring, dtype):
    return core().TileGeom.aligned(w, h, ring, ring, torch.tensor([], dtype=dtype).element_size())


def _full(buf, g):
    return buf.view(g.total_height(), g.pitch)[:, g.x_origin:g.x_origin + g.total_width()]


def _core(buf, g):
    return _full(buf, g)[g.halo_y:g.halo_y + g.height, g.halo_x:g.halo_x + g.width]


def _random_tile(gpu, w, h, ring, dtype, seed):
    """A tile whose core AND ghost ring are random, so held values are neither
    uniform nor zero; the alignment padding stays zero."""
    g = _geom(w, h, ring, dtype)
    gen = torch.Generator(device="cpu").manual_seed(seed)
    full = torch.rand(g.total_height(), g.total_width(), generator=gen, dtype=torch.float64).to(dtype)
    src = torch.zeros(g.alloc_elems(), dtype=dtype, device=gpu)
    _full(src, g).copy_(full)
    return g, full, src


def _ring_mask(g):
    m = torch.ones(g.total_height(), g.total_width(), dtype=torch.bool)
    m[g.halo_y:g.halo_y + g.height, g.halo_x:g.halo_x + g.width] = False
    return m


@pytest.mark.parametrize("w,h,steps,dtype,hold", KERNEL_CASES)
def test_held_kernel_matches_reference(gpu, w, h, steps, dtype, hold):
    g, full, src = _random_tile(gpu, w, h, steps, dtype, w + h + steps)
    dst = torch.full_like(src, -3.0)
    ops.stencil5_tb_held(src, dst, g, steps, 0, w, 0, h, 0.2, 0.2, hold)
    assert hip().last_stencil_dispatch() == "tb_held"
    torch.cuda.synchronize()
    ref = ops.jacobi_held_reference(full, steps, 0.2, 0.2, hold)
    r = steps
    err = (_core(dst, g).cpu().double() - ref[r:r + h, r:r + w].double()).abs().max().item()
    print(f"held kernel {w}x{h} S={steps} {dtype} hold={hold}: max|err| = {err:.3e}")
    assert err <= TOL[dtype]
    out = _full(dst, g).cpu()
    assert (out[_ring_mask(g)] == -3.0).all(), "the kernel wrote outside the core"
    assert (dst.view(g.total_height(), g.pitch)[:, :g.x_origin] == -3.0).all()
    assert (dst.view(g.total_height(), g.pitch)[:, g.x_origin + g.total_width():] == -3.0).all()


@pytest.mark.parametrize("rect", [(0, 20, 12, 188),      # a left strip (tall narrow tiles)
                                  (0, 264, 188, 200),    # a bottom strip (wide flat tiles)
                                  (244, 264, 12, 188)])  # a right strip
def test_held_kernel_sub_rectangle(gpu, rect):
    w, h, steps, hold = 264, 200, 12, 15
    x0, x1, y0, y1 = rect
    g, full, src = _random_tile(gpu, w, h, steps, F32, 77)
    dst = torch.full_like(src, -3.0)
    ops.stencil5_tb_held(src, dst, g, steps, x0, x1, y0, y1, 0.2, 0.2, hold)
    torch.cuda.synchronize()
    ref = ops.jacobi_held_reference(full, steps, 0.2, 0.2, hold)[steps:steps + h, steps:steps + w]
    got = _core(dst, g).cpu()
    assert (got[y0:y1, x0:x1].double() - ref[y0:y1, x0:x1].double()).abs().max().item() <= TOL[F32]
    outside = torch.ones(h, w, dtype=torch.bool)
    outside[y0:y1, x0:x1] = False
    assert (got[outside] == -3.0).all(), "cells outside the rectangle were written"
    assert (_full(dst, g).cpu()[_ring_mask(g)] == -3.0).all()


@pytest.mark.parametrize("w,h,steps,dtype,hold", [KERNEL_CASES[1], KERNEL_CASES[5]])
def test_held_kernel_bitwise_equals_single_steps(gpu, w, h, steps, dtype, hold):
    assert hold == 15  # all sides held: the ring is the same at every level
    g, full, src = _random_tile(gpu, w, h, steps, dtype, 5 * w + steps)
    dst = torch.full_like(src, -3.0)
    ops.stencil5_tb_held(src, dst, g, steps, 0, w, 0, h, 0.2, 0.2, hold)
    a, b = src.clone(), src.clone()  # single steps ping-pong between two buffers that carry the same ring
    for _ in range(steps):
        ops.stencil5_tb_held(a, b, g, 1, 0, w, 0, h, 0.2, 0.2, hold)
        a, b = b, a
    torch.cuda.synchronize()
    assert torch.equal(_core(dst, g), _core(a, g))


@pytest.mark.parametrize("w,h,steps,dtype", [(264, 200, 12, F32), (262, 200, 5, F32), (202, 136, 7, F64)])
def test_hold_none_equals_stencil5_tb(gpu, w, h, steps, dtype):
    g, _, src = _random_tile(gpu, w, h, steps, dtype, 3 * w + steps)
    got, want = torch.full_like(src, -3.0), torch.full_like(src, -3.0)
    ops.stencil5_tb_held(src, got, g, steps, 0, w, 0, h, 0.2, 0.2, 0)
    hip().stencil5_tb(src.data_ptr(), want.data_ptr(), g, steps, 0, w, 0, h, 0.2, 0.2, False, dtype_name(src),
                      _stream(), "auto", False)
    torch.cuda.synchronize()
    assert torch.equal(got, want)


def test_held_kernel_rejects_what_it_cannot_run(gpu):
    g, _, src = _random_tile(gpu, 64, 48, 4, F32, 1)
    dst = torch.zeros_like(src)
    with pytest.raises(Exception, match="ghost ring"):
        ops.stencil5_tb_held(src, dst, g, 5, 0, 64, 0, 48)
    with pytest.raises(Exception, match="multiple of the vector width"):
        ops.stencil5_tb_held(src, dst, g, 4, 2, 64, 0, 48)
    with pytest.raises(Exception, match="out of the core"):
        ops.stencil5_tb_held(src, dst, g, 4, 0, 68, 0, 48)
    g64, _, s64 = _random_tile(gpu, 64, 48, 20, F64, 1)
    with pytest.raises(Exception, match="steps must be in"):
        ops.stencil5_tb_held(s64, torch.zeros_like(s64), g64, 17, 0, 64, 0, 48)


# ------------------------------------------------------------------ solver
def _boundary(w, h, dtype, seed):
    gen = torch.Generator(device="cpu").manual_seed(seed)
    return [torch.rand(n, generator=gen, dtype=torch.float64).to(dtype) for n in (w, w, h, h)]


def _solver(w, h, time_block, dtype, blocked, sum_form=False, seed=3):
    st = Stencil2D(StencilConfig(global_width=w, global_height=h, dims="1x1", dtype=dtype_name(torch.empty(0, dtype=dtype)),
                                 periodic=False, block_fixed_edges=blocked, time_block=time_block, sum_form=sum_form,
                                 seed=seed))
    top, bottom, left, right = _boundary(w, h, dtype, w + h)
    st.set_boundary(top=top, bottom=bottom, left=left, right=right)
    return st, (top, bottom, left, right)


_single_step_runs = {}


def _single_step_core(w, h, iters, dtype):
    """The core after `iters` iterations on today's S = 1 path (computed once)."""
    key = (w, h, iters, dtype)
    if key not in _single_step_runs:
        st, _ = _solver(w, h, 12, dtype, blocked=False)
        assert st.time_block == 1 and st.fixed_edge_note() == ""
        st.run(iters)
        st.synchronize()
        _single_step_runs[key] = st.core_view().clone()
    return _single_step_runs[key]


def _assert_ring_unchanged(st, bnd):
    g = st.geom
    full = st.full_view()
    top, bottom, left, right = (t.to(full.device) for t in bnd)
    hx, hy = g.halo_x, g.halo_y
    assert torch.equal(full[hy - 1, hx:hx + g.width], top)
    assert torch.equal(full[hy + g.height, hx:hx + g.width], bottom)
    assert torch.equal(full[hy:hy + g.height, hx - 1], left)
    assert torch.equal(full[hy:hy + g.height, hx + g.width], right)


@pytest.mark.parametrize("w,h,time_block,iters,dtype", [
    (640, 200, 12, 14, F32),
    (1032, 300, 20, 47, F32),   # pipeline interior, odd split
    (48, 40, 16, 16, F32),      # a 16 x 8 interior inside four strips, one 16-step pass
    (40, 24, 12, 12, F32),      # no interior: the whole core is one frame rectangle
    (400, 264, 16, 35, F64),
])
def test_solver_blocked_equals_single_steps_bitwise(gpu, w, h, time_block, iters, dtype):
    st, bnd = _solver(w, h, time_block, dtype, blocked=True)
    assert st.time_block == time_block and st.solver.time_block() == time_block
    assert st.fixed_edge_note() and "held sides: top,bottom,left,right" in st.fixed_edge_note()
    assert st.solver.held_sides() == 15
    st.run(iters)
    st.synchronize()
    assert max(s for s, _ in st.last_run_blocks()) > 1
    assert "fixed edges" in st.halo_mode()
    assert torch.equal(st.core_view(), _single_step_core(w, h, iters, dtype))
    _assert_ring_unchanged(st, bnd)


def test_solver_blocked_sum_form(gpu):
    w, h, time_block, iters = 640, 200, 12, 14
    st, bnd = _solver(w, h, time_block, F32, blocked=True, sum_form=True)
    assert st.time_block == time_block
    st.run(iters)
    st.synchronize()
    assert st.sum_form_active
    err = (st.core_view().double() - _single_step_core(w, h, iters, F32).double()).abs().max().item()
    print(f"sum-form interior + per-step frame vs S = 1: max|err| = {err:.3e}")
    assert err <= 2e-6
    _assert_ring_unchanged(st, bnd)


def test_solver_blocked_graphs_and_repeated_calls(gpu):
    w, h = 640, 200
    st, bnd = _solver(w, h, 12, F32, blocked=True)
    for n in (7, 33, 1):
        st.run(n)
    st.synchronize()
    assert "fail" not in st.graph_status().lower(), st.graph_status()
    assert torch.equal(st.core_view(), _single_step_core(w, h, 41, F32))
    _assert_ring_unchanged(st, bnd)


@pytest.mark.parametrize("rows_periodic,cols_periodic,hold", [(True, False, 12), (False, True, 3)])
def test_solver_mixed_topology_native(gpu, rows_periodic, cols_periodic, hold):
    """One periodic and one fixed dimension on a 1x1 grid, through the native
    binding (the Python Decomposition takes one flag for both dimensions)."""
    w, h, S, iters = 264, 200, 12, 30
    H, C = hip(), core()
    topo = C.CartTopology(1, 1, rows_periodic, cols_periodic)
    g = _geom(w, h, S, F32)
    gen = torch.Generator(device="cpu").manual_seed(11)
    init = torch.rand(g.total_height(), g.total_width(), generator=gen, dtype=torch.float64).float()
    # The fixed sides' ring is uniform along the periodic dimension, corners
    # included: no exchange fills a ring corner whose diagonal has no rank, and
    # the wrapped rows (columns) read the boundary values there.
    if cols_periodic:
        init[:S, :], init[-S:, :] = 0.25, 0.75
    else:
        init[:, :S], init[:, -S:] = 0.25, 0.75

    def run(blocked):
        a = torch.zeros(g.alloc_elems(), dtype=F32, device=gpu)
        _full(a, g).copy_(init)
        b = a.clone()  # both buffers carry the same ring
        torch.cuda.synchronize()
        s = H.StencilSolver(topo, 0, g, a.data_ptr(), b.data_ptr(), None, "f32", H.HaloBackend.LOCAL, False, True,
                            False, H.StencilKind.JACOBI5, 0.2, 0.2, 1, [], "auto", True, S, sum_form=False,
                            block_fixed_edges=blocked)
        s.run(iters)
        s.synchronize()
        cur = a if s.current() == a.data_ptr() else b
        return s.time_block(), s.held_sides(), s.fixed_edge_note(), _core(cur, g).clone()

    tb1, held1, note1, want = run(False)
    assert (tb1, held1, note1) == (1, 0, "")
    tb, held, note, got = run(True)
    assert tb == S and held == hold and note
    assert torch.equal(got, want)


# -------------------------------------------------------------- multi-rank
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


class _PortTaken(RuntimeError):
    pass


def _launch_once(nprocs, args, timeout):
    port = _free_port()
    procs = []
    for r in range(nprocs):
        env = dict(os.environ)
        env.update(RANK=str(r), WORLD_SIZE=str(nprocs), LOCAL_RANK=str(r), LOCAL_WORLD_SIZE=str(nprocs),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), OMP_NUM_THREADS="1",
                   HSA_ENABLE_IPC_MODE_LEGACY="0")
        procs.append(subprocess.Popen([sys.executable, os.path.join(HERE, "fixed_edge_worker.py"), json.dumps(args)],
                                      env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    results = []
    try:
        for p in procs:
            out, err = p.communicate(timeout=timeout)
            if p.returncode != 0:
                if "EADDRINUSE" in err or "address already in use" in err:
                    raise _PortTaken(err[-500:])
                raise RuntimeError(f"rank failed rc={p.returncode}\n{err[-3000:]}")
            line = [ln for ln in out.splitlines() if ln.startswith("RESULT ")]
            assert line, f"no result\nstdout={out[-2000:]}\nstderr={err[-2000:]}"
            results.append(json.loads(line[-1][len("RESULT "):]))
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
        for p in procs:
            try:
                p.wait(timeout=30)
            except subprocess.TimeoutExpired:
                pass
    return sorted(results, key=lambda r: r["rank"])


def _launch(nprocs, args, timeout=180):
    """Ranks sharing the GPU; only a rendezvous port taken before rank 0 bound
    it (nothing ran yet) is retried."""
    for _ in range(3):
        try:
            return _launch_once(nprocs, args, timeout)
        except _PortTaken:
            continue
    return _launch_once(nprocs, args, timeout)


_one_rank_grids = {}


def _one_rank_grid(dtype, iters):
    if (dtype, iters) not in _one_rank_grids:
        res = _launch(1, {"w": 264, "h": 200, "dims": "1x1", "dtype": dtype, "backend": "local",
                          "block_fixed_edges": False, "time_block": 12, "runs": [iters]})
        assert res[0]["time_block"] == 1 and res[0]["note"] == ""
        _one_rank_grids[(dtype, iters)] = res[0]["grid"]
    return _one_rank_grids[(dtype, iters)]


@pytest.mark.parametrize("dims,time_block,dtype,direct", [
    ("1x2", 20, "f32", False),
    ("2x1", 12, "f32", False),
    ("2x2", 12, "f32", False),
    ("2x3", 5, "f64", False),
    ("2x2", 12, "f32", None),   # the default device-initiated (direct) halo of the IPC backend
])
def test_multi_rank_blocked_equals_one_rank_single_steps(gpu, dims, time_block, dtype, direct):
    rows, cols = (int(x) for x in dims.split("x"))
    iters = 2 * time_block + 3
    res = _launch(rows * cols, {"w": 264, "h": 200, "dims": dims, "dtype": dtype, "backend": "ipc",
                                "block_fixed_edges": True, "time_block": time_block, "direct_halo": direct,
                                "runs": [iters]})
    for r in res:
        assert r["time_block"] == time_block, r
        assert r["note"], r
        assert r["choice"] == "serial" and "fixed edges" in r["reason"], r
        assert r["direct"] == (direct is None), r
        if direct is False:
            assert r["openings"] == ["serial"], r
    # every rank of these grids touches a physical edge; the masks differ by position
    assert len({r["held"] for r in res}) == len(res) or dims in ("1x2", "2x1")
    assert all(r["held"] != 0 for r in res)
    assert res[0]["grid"] == _one_rank_grid(dtype, iters)
