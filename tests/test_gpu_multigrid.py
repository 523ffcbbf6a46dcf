"""Geometric multigrid on the GPU: each of the four HIP kernels bit for bit
against its pure-torch reference (and what it may read and write), the native
solver's V-cycle against the composed reference (graph and eager), its residual
against Stencil2D's, a manufactured Poisson solution, an independent cross-check
against the Chebyshev solver, the errors and the CLI."""
import json
import math
import os
import subprocess
import sys

import pytest
import torch

from cuda_mpi_scratch_amd import core, hip, ops
from cuda_mpi_scratch_amd.models.multigrid2d import Multigrid2D, MultigridConfig
from tests.relaxation_worker import BOUNDARY
from tests.source_worker import make
from tests.test_source_cpu import manufactured

pytestmark = pytest.mark.gpu

DT = {"f32": torch.float32, "f64": torch.float64}
SENTINEL = -3.0
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CACHE = {}


def _geom(w, h, dtype):
    return core().TileGeom.aligned(w, h, 1, 1, torch.tensor([], dtype=dtype).element_size())


def _full(buf, g):
    return buf.view(g.total_height(), g.pitch)[:, g.x_origin:g.x_origin + g.total_width()]


def _core(buf, g):
    return _full(buf, g)[1:1 + g.height, 1:1 + g.width]


def _rand(shape, gen, dtype, amp=1.0):
    return ((torch.rand(*shape, generator=gen, dtype=torch.float64) * 2 - 1) * amp).to(dtype)


def _tile(gpu, g, dtype, full=None, core_vals=None, fill=float("nan")):
    """A flat device tile filled with `fill` (padding included), then the whole
    logical tile (`full`) or only its core (`core_vals`) written."""
    t = torch.full((g.alloc_elems(),), fill, dtype=dtype, device=gpu)
    if full is not None:
        _full(t, g).copy_(full)
    if core_vals is not None:
        _core(t, g).copy_(core_vals)
    return t


def _assert_only_core_written(out, g, want_core, what):
    """The core equals the reference bit for bit, holds no NaN, and everything
    else (ring, alignment padding) still holds the sentinel."""
    have = _core(out, g).cpu()
    n = int((have != want_core).sum())
    print(f"{what}: {n} of {have.numel()} cells differ from the reference")
    assert torch.isfinite(have).all(), "a NaN from a ring or from padding reached a stored cell"
    assert n == 0
    rest = out.clone()
    _core(rest, g).fill_(SENTINEL)
    assert bool((rest == SENTINEL).all()), "the kernel wrote outside the core"


def _fields(w, h, dtype):
    """Per shape and type, made once and left unchanged: u (core and ring random
    in [-1, 1]) and g (core random in [-0.1, 0.1]) on the CPU."""
    key = ("fields", w, h, dtype)
    if key not in _CACHE:
        gen = torch.Generator(device="cpu").manual_seed(1000 * w + h)
        _CACHE[key] = (_rand((h + 2, w + 2), gen, dtype), _rand((h, w), gen, dtype, 0.1))
    return _CACHE[key]


# ------------------------------------------------------------------ smoother
def _smooth_table(w, h, nu):
    """NU different sweeps, so a wrong table index shows: the first levels of the
    grid's 4-level Chebyshev cycle with their weights."""
    t = core().chebyshev_cycle(w, h, 0.2, 0.2, 4)
    return list(t["center"])[:nu], list(t["neighbor"])[:nu], [n / 0.2 for n in t["neighbor"]][:nu]


@pytest.mark.parametrize("nu", [1, 2, 3, 4])
@pytest.mark.parametrize("w,h", [(3, 3), (7, 5), (31, 63), (130, 70), (259, 131)])
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_smoother_is_bitwise_the_reference(gpu, dtype, w, h, nu):
    """The smoother's workgroup stores a 64 x 32 tile (kMgTw x kMgTh): (3, 3) and
    (7, 5) sit inside one tile, narrower than a 16-byte vector or an odd width;
    (31, 63) is one tile wide and two high with a ragged last tile (31 rows);
    (130, 70) has 3 x 3 tiles, the last of each axis ragged (2 columns, 6 rows);
    (259, 131) has 5 x 5 tiles with 3 ragged columns and rows. Each with 1..4
    fused sweeps, on pitch-padded TileGeom.aligned tiles."""
    dt = DT[dtype]
    u, gsrc = _fields(w, h, dt)
    ce, nb, wt = _smooth_table(w, h, nu)
    key = ("smooth", w, h, dtype, nu)
    if key not in _CACHE:
        _CACHE[key] = ops.mg_smooth_reference(u, gsrc, ce, nb, wt)[1:-1, 1:-1].clone()
    g = _geom(w, h, dt)
    u_in = _tile(gpu, g, dt, full=u)          # padding NaN: only core and ring may be read
    src = _tile(gpu, g, dt, core_vals=gsrc)   # ring and padding NaN
    out = _tile(gpu, g, dt, fill=SENTINEL)
    ops.mg_smooth(u_in, out, src, g, ce, nb, wt)
    torch.cuda.synchronize()
    assert hip().last_multigrid_dispatch() == "mg_smooth"
    _assert_only_core_written(out, g, _CACHE[key], f"mg_smooth {dtype} {w}x{h} NU={nu}")
    assert torch.equal(_full(u_in, g).cpu(), u), "the smoother changed its input"


def test_smoother_default_table_and_errors(gpu):
    dt = torch.float64
    w, h = 130, 70
    u, gsrc = _fields(w, h, dt)
    t = ops.mg_smoother_table(0.2, 0.2, 0.8, 2)
    g = _geom(w, h, dt)
    u_in, src, out = _tile(gpu, g, dt, full=u), _tile(gpu, g, dt, core_vals=gsrc), _tile(gpu, g, dt, fill=SENTINEL)
    ops.mg_smooth(u_in, out, src, g, t["center"], t["neighbor"], t["weight"])
    torch.cuda.synchronize()
    want = ops.jacobi_source_per_step_reference(u, gsrc, [0.2, 0.2], [0.2, 0.2], 0.2, hold=15)[1:-1, 1:-1]
    _assert_only_core_written(out, g, want, "mg_smooth default table vs the per-step source reference")
    with pytest.raises(Exception, match="u_in != u_out"):
        ops.mg_smooth(u_in, u_in, src, g, t["center"], t["neighbor"], t["weight"])
    with pytest.raises(Exception, match="sweeps per launch"):
        ops.mg_smooth(u_in, out, src, g, [0.2] * 5, [0.2] * 5, [1.0] * 5)
    with pytest.raises(TypeError):
        ops.mg_smooth(u, u.clone(), gsrc, g, [0.2], [0.2], [1.0])


# ------------------------------------------------------- restrict and prolong
TRANSFER_SHAPES = [(3, 3), (7, 5), (63, 31), (131, 259), (255, 127)]


@pytest.mark.parametrize("w,h", TRANSFER_SHAPES)
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_residual_restrict_is_bitwise_the_reference(gpu, dtype, w, h):
    """A workgroup owns 32 x 16 coarse cells: (3, 3) .. (63, 31) are one (partial)
    tile, (131, 259) is 3 x 9 and (255, 127) 4 x 4 tiles with ragged last ones."""
    dt = DT[dtype]
    u, gsrc = _fields(w, h, dt)
    key = ("restrict", w, h, dtype)
    if key not in _CACHE:
        _CACHE[key] = ops.mg_residual_restrict_reference(u, gsrc, 0.2, 0.2)
    g, gc = _geom(w, h, dt), _geom((w - 1) // 2, (h - 1) // 2, dt)
    u_t, src = _tile(gpu, g, dt, full=u), _tile(gpu, g, dt, core_vals=gsrc)
    out = _tile(gpu, gc, dt, fill=SENTINEL)
    ops.mg_residual_restrict(u_t, src, g, out, gc, 0.2, 0.2)
    torch.cuda.synchronize()
    assert hip().last_multigrid_dispatch() == "mg_residual_restrict"
    _assert_only_core_written(out, gc, _CACHE[key], f"mg_residual_restrict {dtype} {w}x{h}")


@pytest.mark.parametrize("w,h", TRANSFER_SHAPES)
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_prolong_add_is_bitwise_the_reference(gpu, dtype, w, h):
    dt = DT[dtype]
    u, _ = _fields(w, h, dt)
    cw, ch = (w - 1) // 2, (h - 1) // 2
    key = ("prolong", w, h, dtype)
    if key not in _CACHE:
        e = _rand((ch, cw), torch.Generator(device="cpu").manual_seed(7 * w + h), dt)
        _CACHE[key] = (e, ops.mg_prolong_add_reference(u[1:-1, 1:-1], e))
    e, want = _CACHE[key]
    g, gc = _geom(w, h, dt), _geom(cw, ch, dt)
    e_t = _tile(gpu, gc, dt, core_vals=e)                       # ring and padding NaN: e = 0 outside the core
    u_t = _tile(gpu, g, dt, core_vals=u[1:-1, 1:-1], fill=SENTINEL)  # in place: ring and padding hold the sentinel
    ops.mg_prolong_add(e_t, gc, u_t, g)
    torch.cuda.synchronize()
    assert hip().last_multigrid_dispatch() == "mg_prolong_add"
    _assert_only_core_written(u_t, g, want, f"mg_prolong_add {dtype} {w}x{h}")


def test_transfer_kernels_refuse_mismatched_levels(gpu):
    dt = torch.float64
    g, gc = _geom(64, 31, dt), _geom(31, 15, dt)
    a, b = _tile(gpu, g, dt, fill=0.0), _tile(gpu, gc, dt, fill=0.0)
    with pytest.raises(Exception, match="odd fine tile"):
        ops.mg_residual_restrict(a, a, g, b, gc)
    with pytest.raises(Exception, match="odd fine tile"):
        ops.mg_prolong_add(b, gc, a, g)


# --------------------------------------------------------------- coarse solve
@pytest.mark.parametrize("w,h", [(1, 1), (3, 1), (16, 8), (31, 31), (63, 63)])
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_coarse_solve_is_bitwise_the_reference(gpu, dtype, w, h):
    dt = DT[dtype]
    p = ops.mg_coarse_plan(w, h, 0.2, 0.2, 1e-3)
    key = ("coarse", w, h, dtype)
    if key not in _CACHE:
        gsrc = _rand((h, w), torch.Generator(device="cpu").manual_seed(w + 64 * h), dt, 1e-3)
        _CACHE[key] = (gsrc, ops.mg_coarse_solve_reference(gsrc, p["center"], p["neighbor"], p["weight"], p["repeats"]))
    gsrc, want = _CACHE[key]
    g = _geom(w, h, dt)
    src, out = _tile(gpu, g, dt, core_vals=gsrc), _tile(gpu, g, dt, fill=SENTINEL)
    ops.mg_coarse_solve(src, out, g, p["center"], p["neighbor"], p["weight"], p["repeats"])
    torch.cuda.synchronize()
    assert hip().last_multigrid_dispatch() == "mg_coarse_solve"
    _assert_only_core_written(out, g, want, f"mg_coarse_solve {dtype} {w}x{h} ({p['repeats']} x 32 sweeps)")
    # it solves: the residual of e against g fell by the planned factor (fp64)
    if dtype == "f64" and w * h > 1:
        full = torch.zeros(h + 2, w + 2, dtype=dt)
        full[1:-1, 1:-1] = want
        r = ops.mg_residual_reference(full, gsrc)
        assert float(torch.linalg.vector_norm(r)) <= 2e-3 * float(torch.linalg.vector_norm(gsrc))


def test_coarse_solve_refuses_a_grid_above_its_lds(gpu):
    dt = torch.float32
    g = _geom(64, 8, dt)
    a = _tile(gpu, g, dt, fill=0.0)
    with pytest.raises(Exception, match="at most 63"):
        ops.mg_coarse_solve(a, a.clone(), g, [0.2], [0.2], [1.0], 1)


# --------------------------------------------------------------------- solver
def _problem(w, h, dtype, device, **kw):
    """Non-zero boundaries on all sides, a random start and a random source."""
    m = Multigrid2D(MultigridConfig(width=w, height=h, dtype=dtype, **kw), device=device)
    gen = torch.Generator(device="cpu").manual_seed(w + 3 * h)
    m.set_boundary(top=1.0, bottom=_rand((w,), gen, torch.float64), left=torch.linspace(1.0, 0.0, h, dtype=torch.float64),
                   right=-0.5)
    m.set_field(_rand((h, w), gen, torch.float64))
    m.set_source(_rand((h, w), gen, torch.float64, 1e-3))
    return m


@pytest.mark.parametrize("nu", [(2, 2), (1, 3)])
@pytest.mark.parametrize("w,h", [(127, 63), (255, 255), (35, 67)])
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_vcycle_is_bitwise_the_composed_reference_graph_and_eager(gpu, dtype, w, h, nu):
    kw = dict(nu_pre=nu[0], nu_post=nu[1])
    key = ("vcycle", w, h, dtype, nu)
    if key not in _CACHE:
        ref = _problem(w, h, dtype, "cpu", **kw)
        start = ref.full()
        ref.vcycle(2)
        _CACHE[key] = (start, ref.full())
    start, want = _CACHE[key]
    for graph in (True, False):
        m = _problem(w, h, dtype, "cuda", graph=graph, **kw)
        assert m.solver is not None and m.levels() == ops.mg_plan_levels(w, h)
        assert torch.equal(m.full().cpu(), start), "set_boundary / set_field differ between the backends"
        m.vcycle(2)
        got = m.full().cpu()
        n = int((got != want).sum())
        print(f"V{nu} {dtype} {w}x{h} graph={graph} ({m.graph_status()}, {m.solver.launches_per_cycle()} launches): "
              f"{n} of {got.numel()} cells differ")
        assert m.graph_status() == ("captured" if graph else "off")
        assert n == 0


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_residual_is_bitwise_the_stencil_solvers(gpu, dtype):
    """Same field, source and boundary: fp64 against Stencil2D(source=True).residual().
    The fp32 source solver needs a width of whole 4-cell vectors, which no multigrid
    size has (they are odd), so fp32 compares with the kernel Stencil2D.residual()
    runs, ops.stencil5_residual, on a tile of another geometry (a ring 4 deep)."""
    w, h = 127, 63
    gen = torch.Generator(device="cpu").manual_seed(9)
    field, src = _rand((h, w), gen, DT[dtype]), _rand((h, w), gen, DT[dtype], 0.01)
    m = Multigrid2D(MultigridConfig(width=w, height=h, dtype=dtype), device="cuda")
    m.set_boundary(**BOUNDARY)
    m.set_field(field)
    m.set_source(src)
    b = m.residual()
    if dtype == "f64":
        st = make({"w": w, "h": h, "dtype": dtype, "time_block": 16, "zero": True})
        st.core_view().copy_(field)
        st.set_source(src)
        a = st.residual()
    else:
        g = core().TileGeom.aligned(w, h, 4, 4, 4)
        full = torch.zeros(g.total_height(), g.total_width(), dtype=DT[dtype])
        full[3:-3, 3:-3] = m.full().cpu()
        u_t, s_t = _tile(gpu, g, DT[dtype], fill=0.0), _tile(gpu, g, DT[dtype])
        _full(u_t, g).copy_(full)
        _full(s_t, g)[4:-4, 4:-4].copy_(src)
        linf, sumsq = ops.stencil5_residual(u_t, g, 0.2, 0.2, source=s_t)
        a = {"linf": linf, "l2": math.sqrt(sumsq), "cells": w * h}
    print(f"residual {dtype}: stencil {a}, Multigrid2D {b}")
    assert a["l2"] > 0 and a == b


def test_no_source_nonzero_boundaries_converge_on_the_device(gpu):
    m = Multigrid2D(MultigridConfig(width=255, height=127, dtype="f64"), device="cuda")
    m.set_boundary(**BOUNDARY)
    m.set_source(1e-3)
    m.set_source(None)
    r0 = m.residual()["l2"]
    out = m.solve(1e-8 * r0, 14)
    l2 = [c[2] for c in out["history"]]
    print(f"no source 255x127: {out['cycles']} cycles, factors {[round(b / a, 4) for a, b in zip(l2, l2[1:])]}")
    assert out["converged"] and out["cycles"] <= 11, out
    # the source is gone: the residual is that of A u - u on the solver's own field
    _, l2_ref = ops.residual5_reference(m.full().cpu(), 1, 0.2, 0.2)
    assert out["residual"] == pytest.approx(l2_ref, rel=1e-9)


def test_fp32_solve_stalls_at_its_floor_like_the_reference(gpu):
    a, b = _problem(127, 63, "f32", "cuda"), _problem(127, 63, "f32", "cpu")
    oa, ob = a.solve(0.0, 40), b.solve(0.0, 40)
    print(f"fp32 127x63: device {oa['reason']} after {oa['cycles']} cycles, reference {ob['reason']} after {ob['cycles']}")
    assert oa["reason"] == ob["reason"] and oa["cycles"] == ob["cycles"]
    # the fields are bitwise equal; the norms differ only in the order of their sums
    for (ca, la, sa), (cb, lb, sb) in zip(oa["history"], ob["history"]):
        assert ca == cb and la == lb and sa == pytest.approx(sb, rel=1e-9)
    assert oa["reason"] == "stalled" or oa["converged"]


def test_manufactured_poisson_solution_on_the_device(gpu):
    w, h, tol = 127, 63, 1e-10
    u_star, g, a = manufactured(w, h)
    m = Multigrid2D(MultigridConfig(width=w, height=h, dtype="f64"), device="cuda")
    m.set_source(g)
    out = m.solve(tol, 30)
    err = float(torch.linalg.vector_norm(m.field().cpu() - u_star))
    print(f"manufactured {w}x{h} on the device: {out['cycles']} cycles, l2 residual {out['residual']:.3e}, "
          f"||u - u*||_2 {err:.3e}, bound {tol / a:.3e}")
    assert out["converged"], out["reason"]
    assert err <= tol / a


def test_cross_check_against_the_chebyshev_solver(gpu):
    """Two independent solvers of one problem: ||u_mg - u_cheb||_2 <= (||r_mg||_2 +
    ||r_cheb||_2) / a <= 2e-10 / a, and multigrid gets there in fewer fine-grid
    sweep equivalents than Chebyshev takes iterations."""
    w, h, tol, M = 127, 63, 1e-10, 16
    _, _, a = manufactured(w, h)
    src = _rand((h, w), torch.Generator(device="cpu").manual_seed(21), torch.float64, 0.01)
    st = make({"w": w, "h": h, "dtype": "f64", "time_block": M, "zero": True})
    st.set_source(src)
    cheb = st.run_until(tol, M * 600, norm="l2")
    m = Multigrid2D(MultigridConfig(width=w, height=h, dtype="f64"), device="cuda")
    m.set_boundary(**BOUNDARY)
    m.set_source(src)
    out = m.solve(tol, 30)
    diff = float(torch.linalg.vector_norm(m.field() - st.core_view()))
    sweeps = out["cycles"] * (m.cfg.nu_pre + m.cfg.nu_post) * 4 / 3
    print(f"cross-check {w}x{h}: multigrid {out['cycles']} cycles ({sweeps:.1f} sweep equivalents, residual "
          f"{out['residual']:.3e}), Chebyshev {cheb['iterations']} iterations (residual {cheb['residual']:.3e}), "
          f"||u_mg - u_cheb||_2 {diff:.3e}, bound {2 * tol / a:.3e}")
    assert cheb["converged"] and out["converged"], (cheb["reason"], out["reason"])
    assert diff <= 2 * tol / a
    assert sweeps < cheb["iterations"]


# -------------------------------------------------------------- errors, CLI
def test_errors_on_the_device(gpu):
    from cuda_mpi_scratch_amd.parallel import DistContext

    with pytest.raises(ValueError, match="2047"):
        Multigrid2D(MultigridConfig(width=2048, height=2048), device="cuda")
    with pytest.raises(ValueError, match="pure Laplace"):
        hip().MultigridSolver(127, 127, "f64", 0.3, 0.2)
    with pytest.raises(ValueError, match="pure Laplace"):
        MultigridConfig(width=127, height=127, c_center=0.3)
    with pytest.raises(ValueError, match="one process"):
        Multigrid2D(MultigridConfig(width=127, height=127), DistContext(rank=0, world_size=2), device="cuda")
    m = Multigrid2D(MultigridConfig(width=127, height=63), device="cuda")
    with pytest.raises(ValueError, match="shape"):
        m.set_source(torch.zeros(127, 63))
    with pytest.raises(ValueError, match="norm"):
        m.solve(1e-8, 5, norm="l1")


def test_cli_solves_and_writes_its_json(gpu, tmp_path):
    path = tmp_path / "mg.json"
    cmd = [sys.executable, "-m", "cuda_mpi_scratch_amd.models.multigrid2d", "--size", "255x255", "--dtype", "f64",
           "--source", "1e-6", "--tol", "1e-8", "--json", str(path)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    rec = json.loads(path.read_text().splitlines()[-1])
    assert rec == json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert rec["converged"] and rec["cycles"] <= 14 and rec["residual"] <= 1e-8
    assert rec["graph"] == "captured" and rec["levels"][0] == [255, 255] and rec["levels"][-1] == [31, 31]
    assert rec["device"].startswith("cuda")
