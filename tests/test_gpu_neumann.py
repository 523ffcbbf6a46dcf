"""Neumann sides on the GPU: the CG kernels and every preconditioner kernel bit
for bit against their pure-torch references under each set of ghost codes (the
all-Dirichlet set included, so the new code paths are also held to the earlier
references), and the two native solvers: exact discrete solutions, a dense
direct solve, the CPU twin's iteration counts, independence of the graph and of
the host's cadence, a repeated solve, fp32, the errors and the CLI.

Everywhere: padding, ring corners and whatever ring cell a launch may not read
hold NaN (the ring of a mirror or reflecting side of the preconditioner, the
whole ring of the tiles cg_apply reads), outputs start as a sentinel, and
nothing outside the core may be written."""
import json
import math
import os
import subprocess
import sys

import pytest
import torch

from cuda_mpi_scratch_amd import hip, ops
from cuda_mpi_scratch_amd.models.cg2d import CgConfig, ConjugateGradient2D
from cuda_mpi_scratch_amd.models.pcg2d import MultigridPcg2D, PcgConfig
from tests.test_gpu_cg import SHAPES, _fields as _cg_fields, _same_bits, _sum_check
from tests.test_gpu_multigrid import (DT, SENTINEL, _assert_only_core_written, _fields, _geom, _rand, _smooth_table,
                                      _tile)
from tests.test_gpu_pcg import FINE
from tests.test_neumann_cpu import ALL, direct_solution, exact_cases, level0, neumann_problem

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")
SIDE_SETS = [(), ("left",), ("right",), ("top",), ("bottom",), ALL]
# (top, bottom, left, right): the all-ring set, one near mirror per axis, all mirrors, and a mirror facing a reflection.
CODE_SETS = [(0, 0, 0, 0), (1, 0, 0, 0), (0, 0, 1, 0), (1, 1, 1, 1), (0, 0, 1, -1), (1, -1, 0, 0)]


def _poison_corners(full):
    full = full.clone()
    full[0, 0] = full[0, -1] = full[-1, 0] = full[-1, -1] = NAN
    return full


def _poison_coded_ring(full, codes):
    """A copy of `full` with NaN in the corners and in the ring of every coded side: those ghosts come from the core."""
    full = _poison_corners(full)
    t, b, l, r = codes
    if t:
        full[0, :] = NAN
    if b:
        full[-1, :] = NAN
    if l:
        full[:, 0] = NAN
    if r:
        full[:, -1] = NAN
    return full


# ----------------------------------------------------------------- CG kernels
@pytest.mark.parametrize("w,h", SHAPES + [(1, 1), (1, 5), (5, 1)])
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_start_kernels_are_bitwise_the_reference(gpu, dtype, w, h):
    """cg_start and pcg_start under every side set: the ring of a Neumann side
    holds random differences d, the ghost is edge + d. (1, 1), (1, 5), (5, 1):
    one cell whose four ghosts all mirror it, and single rows / columns where the
    top and the bottom (left and right) ghost belong to the same cell."""
    dt = DT[dtype]
    f = _cg_fields(w, h, dt)
    c0, c1 = 0.5, 0.1
    g = _geom(w, h, dt)
    u = _tile(gpu, g, dt, full=_poison_corners(f["u"]))
    src = _tile(gpu, g, dt, core_vals=f["g"])
    for neumann in SIDE_SETS:
        want, _, linf = ops.cg_start_reference(f["u"], f["g"], c0, c1, neumann=neumann)
        if not neumann:
            assert torch.equal(want, ops.cg_start_reference(f["u"], f["g"], c0, c1)[0])
        r, p = _tile(gpu, g, dt, fill=SENTINEL), _tile(gpu, g, dt, fill=SENTINEL)
        ws = ops.CgWorkspace(g, gpu)
        ws.write(tol=0.0, max_iters=9, norm="l2", iteration=5, beta=3.0, status=2)
        ops.cg_start(u, src, r, p, g, c0, c1, ws, neumann=neumann)
        torch.cuda.synchronize()
        assert hip().last_cg_dispatch() == "cg_start"
        _assert_only_core_written(r, g, want, f"cg_start r {dtype} {w}x{h} {neumann}")
        _assert_only_core_written(p, g, want, f"cg_start p {dtype} {w}x{h} {neumann}")
        sc = ws.read()
        _sum_check(f"cg_start rr {dtype} {w}x{h} {neumann}", sc["rr"], want.double() ** 2)
        assert sc["linf"] == linf and (sc["iteration"], sc["status"]) == (0, 0) and int(ws.counter.item()) == 0
        r2 = _tile(gpu, g, dt, fill=SENTINEL)
        ws2 = ops.PcgWorkspace(g, gpu)
        ws2.write(tol=0.0, max_iters=9, norm="l2", iteration=5, rz=4.0, status=2)
        ops.pcg_start(u, src, r2, g, c0, c1, ws2, neumann=neumann)
        torch.cuda.synchronize()
        assert hip().last_cg_dispatch() == "pcg_start"
        _assert_only_core_written(r2, g, want, f"pcg_start r {dtype} {w}x{h} {neumann}")
        sc = ws2.read()
        assert sc["linf"] == linf and (sc["rz"], sc["iteration"], sc["status"]) == (0.0, 0, 0)
        assert int(ws2.counter.item()) == 0


@pytest.mark.parametrize("beta", [0.0, 0.37])
@pytest.mark.parametrize("w,h", SHAPES + [(1, 1), (1, 5), (5, 1)])
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_apply_kernels_are_bitwise_the_reference(gpu, dtype, w, h, beta):
    """cg_apply and pcg_apply: the ghost of a mirror side is the edge cell of p_new
    itself; the rings of r and p_old hold NaN and are never loaded. (259, 131) and
    (5, 2090) have several row bands and column groups: only the global edges
    mirror."""
    dt = DT[dtype]
    f = _cg_fields(w, h, dt)
    c0, c1 = 0.5, 0.1
    g = _geom(w, h, dt)
    r, p_old = _tile(gpu, g, dt, core_vals=f["r"]), _tile(gpu, g, dt, core_vals=f["p"])
    for neumann in SIDE_SETS:
        want_p, want_q, _ = ops.cg_apply_reference(f["r"], f["p"], beta, c0, c1, neumann=neumann)
        if not neumann:
            assert torch.equal(want_q, ops.cg_apply_reference(f["r"], f["p"], beta, c0, c1)[1])
        for name, launch, ws in (("cg_apply", ops.cg_apply, ops.CgWorkspace(g, gpu)),
                                 ("pcg_apply", ops.pcg_apply, ops.PcgWorkspace(g, gpu))):
            p_new, q = _tile(gpu, g, dt, fill=SENTINEL), _tile(gpu, g, dt, fill=SENTINEL)
            ws.write(beta=beta, rr=1.25, tol=0.0, max_iters=100, iteration=3, **({"rz": 1.25} if name[0] == "p" else {}))
            launch(r, p_old, p_new, q, g, c0, c1, ws, neumann=neumann)
            torch.cuda.synchronize()
            assert hip().last_cg_dispatch() == name
            _assert_only_core_written(p_new, g, want_p, f"{name} p_new {dtype} {w}x{h} beta={beta} {neumann}")
            _assert_only_core_written(q, g, want_q, f"{name} q {dtype} {w}x{h} beta={beta} {neumann}")
            sc = ws.read()
            _sum_check(f"{name} pq {dtype} {w}x{h} {neumann}", sc["pq"], want_p.double() * want_q.double())
            if sc["pq"] > 0:
                assert sc["alpha"] == 1.25 / sc["pq"] and sc["status"] == 0
            assert int(ws.counter.item()) == 0


# ------------------------------------------------------------------ smoother
@pytest.mark.parametrize("nu", [1, 2, 3, 4])
@pytest.mark.parametrize("w,h", [(1, 1), (2, 2), (3, 3), (64, 32), (65, 33), (63, 31), (130, 70)])
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_smoother_with_codes_is_bitwise_the_reference(gpu, dtype, w, h, nu):
    """test_gpu_pcg's smoother shapes (the ghost beside the first cells, on a
    tile's last column / row, in a neighbour's apron) under every code set: a
    mirror ghost on a near side lives in row -1 / column -1 of the first tile's
    apron. Plain and from zero (+0 beside a mirror, -0 beside a reflection)."""
    dt = DT[dtype]
    u, gsrc = _fields(w, h, dt)
    ce, nb, wt = _smooth_table(w, h, nu)
    g = _geom(w, h, dt)
    src = _tile(gpu, g, dt, core_vals=gsrc)
    for codes in CODE_SETS:
        want = ops.mgp_smooth_reference(u, gsrc, ce, nb, wt, sides=codes)[1:-1, 1:-1].clone()
        if codes == (0, 0, 0, 0):
            assert torch.equal(want, ops.mg_smooth_reference(u, gsrc, ce, nb, wt)[1:-1, 1:-1])
        u_in = _tile(gpu, g, dt, full=_poison_coded_ring(u, codes))
        out = _tile(gpu, g, dt, fill=SENTINEL)
        ops.mgp_smooth(u_in, out, src, g, ce, nb, wt, sides=codes)
        torch.cuda.synchronize()
        assert hip().last_pcg_dispatch() == "mgp_smooth"
        _assert_only_core_written(out, g, want, f"mgp_smooth {dtype} {w}x{h} NU={nu} codes {codes}")
        want0 = ops.mgp_smooth_reference(torch.zeros_like(u), gsrc, ce, nb, wt, sides=codes)[1:-1, 1:-1].clone()
        out0 = _tile(gpu, g, dt, fill=SENTINEL)
        ops.mgp_smooth(None, out0, src, g, ce, nb, wt, sides=codes)
        torch.cuda.synchronize()
        assert hip().last_pcg_dispatch() == "mgp_smooth_zero"
        _assert_only_core_written(out0, g, want0, f"mgp_smooth from zero {dtype} {w}x{h} NU={nu} codes {codes}")


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_smoother_dot_epilogue_with_mirrors(gpu, dtype):
    dt = DT[dtype]
    w, h, codes = 130, 70, (1, 1, 1, 1)
    u, gsrc = _fields(w, h, dt)
    ce, nb, wt = _smooth_table(w, h, 2)
    want = ops.mgp_smooth_reference(u, gsrc, ce, nb, wt, sides=codes)[1:-1, 1:-1].clone()
    g = _geom(w, h, dt)
    u_in = _tile(gpu, g, dt, full=_poison_coded_ring(u, codes))
    src = _tile(gpu, g, dt, core_vals=gsrc)
    ws = ops.PcgWorkspace(g, gpu)
    out = _tile(gpu, g, dt, fill=SENTINEL)
    ws.write(rz=2.0, beta=7.0, iteration=3, status=0, rr=1.5, max_iters=9)
    ops.mgp_smooth(u_in, out, src, g, ce, nb, wt, ws=ws, sides=codes)
    torch.cuda.synchronize()
    assert hip().last_pcg_dispatch() == "mgp_smooth_dot"
    _assert_only_core_written(out, g, want, f"mgp_smooth dot {dtype} {w}x{h} codes {codes}")
    sc = ws.read()
    _sum_check(f"mgp_smooth rz {dtype} {w}x{h}", sc["rz"], gsrc.double() * want.double())
    assert sc["beta"] == sc["rz"] / 2.0 and int(ws.counter.item()) == 0


# ------------------------------------------------- restriction, prolongation
TRANSFER = FINE + [(65, 34), (34, 65)]  # FINE has no odd height


def test_transfer_shapes_cover_both_parities():
    assert {w % 2 for w, _ in TRANSFER} == {0, 1} and {h % 2 for _, h in TRANSFER} == {0, 1}


@pytest.mark.parametrize("w,h", TRANSFER)
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_restriction_with_codes_is_bitwise_the_reference(gpu, dtype, w, h):
    """The codes are the FINE level's. Under a mirror side the residual reads the
    mirrored ghost and the row / column whose outer coarse neighbour is that
    ghost is staged twice: row 0 (column 0) always, the last one on an odd side
    only."""
    dt = DT[dtype]
    u, gsrc = _fields(w, h, dt)
    c0, c1 = 0.15, 0.2
    g, gc = _geom(w, h, dt), _geom(w // 2, h // 2, dt)
    src = _tile(gpu, g, dt, core_vals=gsrc)
    for codes in CODE_SETS:
        want = ops.mgp_residual_restrict_reference(u, gsrc, c0, c1, sides=codes)
        if codes == (0, 0, 0, 0):
            assert torch.equal(want, ops.mgp_residual_restrict_reference(u, gsrc, c0, c1))
        ut = _tile(gpu, g, dt, full=_poison_coded_ring(u, codes))
        out = _tile(gpu, gc, dt, fill=SENTINEL)
        ops.mgp_residual_restrict(ut, src, g, out, gc, c0, c1, sides=codes)
        torch.cuda.synchronize()
        assert hip().last_pcg_dispatch() == "mgp_residual_restrict"
        _assert_only_core_written(out, gc, want, f"mgp_residual_restrict {dtype} {w}x{h} codes {codes}")


@pytest.mark.parametrize("w,h", TRANSFER)
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_prolongation_with_codes_is_bitwise_the_reference(gpu, dtype, w, h):
    """A mirror side clamps the coarse index (fine row 0 beside a mirror top gets
    e[0] itself); ring and reflect sides keep 0. Only the core of e is read."""
    dt = DT[dtype]
    u, _ = _fields(w, h, dt)
    ch, cw = h // 2, w // 2
    e = _rand((ch, cw), torch.Generator(device="cpu").manual_seed(7 * w + h), dt)
    g, gc = _geom(w, h, dt), _geom(cw, ch, dt)
    et = _tile(gpu, gc, dt, core_vals=e)
    for codes in CODE_SETS:
        want = ops.mgp_prolong_add_reference(u[1:-1, 1:-1], e, sides=codes)
        if 1 not in codes:
            assert torch.equal(want, ops.mgp_prolong_add_reference(u[1:-1, 1:-1], e))
        ut = _tile(gpu, g, dt, core_vals=u[1:-1, 1:-1], fill=SENTINEL)
        ops.mgp_prolong_add(et, gc, ut, g, sides=codes)
        torch.cuda.synchronize()
        assert hip().last_pcg_dispatch() == "mgp_prolong_add"
        _assert_only_core_written(ut, g, want, f"mgp_prolong_add {dtype} {w}x{h} codes {codes}")


# -------------------------------------------------------------- coarse solve
@pytest.mark.parametrize("w,h", [(1, 1), (16, 16), (31, 1), (63, 63)])
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_coarse_solve_with_codes_is_bitwise_the_reference(gpu, dtype, w, h):
    """test_gpu_pcg's coarse shapes, two repeats of the level's own plan (the
    32-point cycle on the mirror interval; all four mirrors need a screened
    c_center), without and with the dot epilogue."""
    dt = DT[dtype]
    gsrc = _fields(w, h, dt)[1]
    g = _geom(w, h, dt)
    src = _tile(gpu, g, dt, core_vals=gsrc)
    for codes in CODE_SETS:
        c0 = 0.15 if codes == (1, 1, 1, 1) else 0.2
        level = {"width": w, "height": h, "reflect_rows": codes[1] == -1, "reflect_cols": codes[3] == -1, "c_center": c0,
                 "top": codes[0], "bottom": codes[1], "left": codes[2], "right": codes[3]}
        plan = ops.pcg_coarse_plan(level, 0.2, 1e-3)
        want = ops.mgp_coarse_solve_reference(gsrc, plan["center"], plan["neighbor"], plan["weight"], 2, sides=codes)
        out = _tile(gpu, g, dt, fill=SENTINEL)
        ops.mgp_coarse_solve(src, out, g, plan["center"], plan["neighbor"], plan["weight"], 2, sides=codes)
        torch.cuda.synchronize()
        assert hip().last_pcg_dispatch() == "mgp_coarse_solve"
        _assert_only_core_written(out, g, want, f"mgp_coarse_solve {dtype} {w}x{h} codes {codes}")
        ws = ops.PcgWorkspace(g, gpu)
        ws.write(rz=0.5, iteration=2, status=0, max_iters=9)
        out2 = _tile(gpu, g, dt, fill=SENTINEL)
        ops.mgp_coarse_solve(src, out2, g, plan["center"], plan["neighbor"], plan["weight"], 2, ws=ws, sides=codes)
        _assert_only_core_written(out2, g, want, f"mgp_coarse_solve dot {dtype} {w}x{h} codes {codes}")
        sc = ws.read()
        _sum_check(f"mgp_coarse_solve rz {dtype} {w}x{h} codes {codes}", sc["rz"], gsrc.double() * want.double())
        assert sc["beta"] == sc["rz"] / 0.5


def test_launchers_refuse_bad_codes(gpu):
    dt = torch.float64
    g, gc = _geom(64, 32, dt), _geom(32, 16, dt)
    a, b, c, d = (_tile(gpu, g, dt, fill=0.0) for _ in range(4))
    e = _tile(gpu, gc, dt, fill=0.0)
    with pytest.raises(Exception, match="near side"):
        ops.mgp_smooth(a, b, c, g, [0.2], [0.2], [1.0], sides=(-1, 0, 0, 0))
    with pytest.raises(Exception, match="near side"):
        ops.mgp_residual_restrict(a, b, g, e, gc, sides=(0, 0, -1, 0))
    with pytest.raises(Exception, match="ring \\(0\\) or mirror"):
        hip().cg_apply(a.data_ptr(), b.data_ptr(), c.data_ptr(), d.data_ptr(), g, 0.2, 0.2,
                       *ops.CgWorkspace(g, gpu)._ptrs(), "f64", 0, (0, -1, 0, 0))
    with pytest.raises(ValueError, match="unknown side"):
        ops.cg_start(a, b, c, d, g, 0.2, 0.2, ops.CgWorkspace(g, gpu), neumann=("north",))


# --------------------------------------------------------------------- solvers
MODELS = [(ConjugateGradient2D, CgConfig), (MultigridPcg2D, PcgConfig)]


@pytest.mark.parametrize("model,config", MODELS)
@pytest.mark.parametrize("w,h", [(100, 37), (130, 70)])
def test_exact_discrete_solutions_on_the_device(gpu, w, h, model, config):
    """The three exact solutions of test_neumann_cpu, fp64, l2 <= 1e-11: ||u - u*||_2
    <= tol / a with the level-0 a. The reported residual is the operator's own
    (the start kernel's), and agrees with the CPU reference on the same field."""
    tol = 1e-11
    for name, kw, boundary, source, expect in exact_cases(w, h):
        cfg = config(width=w, height=h, dtype="f64", **kw)
        m = model(cfg, device="cuda")
        assert m.solver is not None
        m.set_boundary(**boundary)
        m.set_source(source)
        out = m.solve(tol, 4 * w * h)
        a = ops.pcg_coarse_interval(level0(w, h, cfg.c_center, cfg.c_neighbor, cfg.neumann), cfg.c_neighbor)[0]
        err = float(torch.linalg.vector_norm(m.field().cpu() - expect))
        src = torch.zeros(h, w, dtype=torch.float64) if source is None else torch.full((h, w), source, dtype=torch.float64)
        _, l2 = ops.residual5_reference(ops.ghosted(m.full().cpu(), cfg.neumann), 1, cfg.c_center, cfg.c_neighbor,
                                        source=src)
        print(f"{model.__name__} ({name}) {w}x{h} {cfg.neumann}: {out['iterations']} iterations, residual "
              f"{out['residual']:.3e} (recomputed {l2:.3e}), error {err:.3e}, bound {tol / a:.3e}; {m.note()}")
        assert out["converged"] and out["residual"] <= tol, out["reason"]
        # The two residuals are different expressions of the same cells: each is a handful of roundings
        # (at most 8 here) of terms no larger than max |u|, so their l2 norms differ by at most that per cell.
        floor = 8 * 2.0 ** -53 * math.sqrt(w * h) * float(m.full().abs().max())
        assert l2 <= tol + floor and abs(out["residual"] - l2) <= floor
        assert out["residual"] == m.residual()["l2"]
        assert err <= (tol / a) * (1 + 1e-6)
        assert "Neumann sides " + ", ".join(cfg.neumann) in m.note()


@pytest.mark.parametrize("model,config", MODELS)
@pytest.mark.parametrize("c0,c1", [(0.2, 0.2), (0.5, 0.1)])
@pytest.mark.parametrize("neumann", [("left",), ("right", "bottom")])
def test_solvers_against_the_dense_direct_solve(gpu, neumann, c0, c1, model, config):
    w, h, tol = 40, 24, 1e-11
    prob = neumann_problem(w, h)
    m = model(config(width=w, height=h, dtype="f64", c_center=c0, c_neighbor=c1, neumann=neumann), device="cuda")
    m.set_boundary(top=prob["top"], bottom=prob["bottom"], left=prob["left"], right=prob["right"])
    m.set_field(prob["field"])
    m.set_source(prob["source"])
    out = m.solve(tol, 4 * w * h)
    a = ops.pcg_coarse_interval(level0(w, h, c0, c1, neumann), c1)[0]
    err = float(torch.linalg.vector_norm(m.field().cpu() - direct_solution(w, h, c0, c1, prob, neumann)))
    print(f"{model.__name__} {neumann} ({c0}, {c1}): {out['iterations']} iterations, residual {out['residual']:.3e}, "
          f"error {err:.3e}, bound {tol / a:.3e}")
    assert out["converged"] and out["residual"] <= tol, out["reason"]
    assert err <= (tol / a) * (1 + 1e-6)


@pytest.mark.parametrize("w,h", [(256, 256), (250, 250), (100, 37)])
def test_iteration_count_is_the_cpu_twins(gpu, w, h):
    """f = 1, zero ring, fp64, l2 <= 1e-8, left and right insulated: held the way
    test_gpu_pcg holds the all-Dirichlet count (the cells are the twin's bit for
    bit given the same scalars, the sums differ in term order: within 1)."""
    neumann = ("left", "right")
    twin = ops.pcg_reference(torch.zeros(h + 2, w + 2, dtype=torch.float64), torch.ones(h, w, dtype=torch.float64),
                             tol=1e-8, max_iters=100, neumann=neumann)
    m = MultigridPcg2D(PcgConfig(width=w, height=h, dtype="f64", neumann=neumann), device="cuda")
    m.set_source(1.0)
    out = m.solve(1e-8, 100)
    diff = float((m.full().cpu() - twin["full"]).abs().max())
    print(f"{w}x{h} {neumann}: device {out['iterations']} iterations (residual {out['residual']:.3e}), twin "
          f"{twin['iterations']} (residual {twin['residual']:.3e}); max |u_gpu - u_twin| {diff:.3e} of "
          f"{float(twin['full'].abs().max()):.3e}")
    assert twin["converged"] and out["converged"], (twin["reason"], out["reason"])
    assert abs(out["iterations"] - twin["iterations"]) <= 1
    assert m.levels == ops.pcg_plan_levels(w, h, neumann=neumann) and len(m.solver.levels()) == len(m.levels)


def _ring_model(model, config, w, h, dtype, **kw):
    m = model(config(width=w, height=h, dtype=dtype, neumann=("left", "top"), **kw), device="cuda")
    gen = torch.Generator(device="cpu").manual_seed(w + 3 * h)
    m.set_boundary(top=_rand((w,), gen, torch.float64, 0.1), bottom=_rand((w,), gen, torch.float64),
                   left=_rand((h,), gen, torch.float64, 0.1), right=-0.5)
    m.set_field(_rand((h, w), gen, torch.float64))
    m.set_source(_rand((h, w), gen, torch.float64, 1e-3))
    return m


@pytest.mark.parametrize("model,config,every", [(ConjugateGradient2D, CgConfig, (8, 32)), (MultigridPcg2D, PcgConfig, (2, 4))])
def test_the_graph_and_the_cadence_change_no_bit_and_a_second_solve_repeats(gpu, model, config, every):
    """250 x 130 with fluxes through the left and the top side: graph against eager
    and two check_every values give identical bits, and after set_field(0) a
    second solve repeats the first (nothing leaks through the scratch tiles the
    residual uses)."""
    w, h, tol = 250, 130, 1e-9
    first = None
    for graph in (True, False):
        for ev in every:
            m = _ring_model(model, config, w, h, "f64", graph=graph, check_every=ev)
            m.set_field(0.0)
            out = m.solve(tol, 5000)
            got = m.full()
            assert out["converged"], out["reason"]
            assert m.graph_status() == ("captured" if graph else "off")
            if first is None:
                first = (got, out["iterations"], out["residual"], out["restarts"])
            assert _same_bits(got, first[0]), "the field depends on the cadence or on the graph"
            assert (out["iterations"], out["residual"], out["restarts"]) == first[1:]
            m.set_field(0.0)
            again = m.solve(tol, 5000)
            assert _same_bits(m.full(), first[0]) and again["iterations"] == first[1] and again["residual"] == first[2]
    print(f"{model.__name__} {w}x{h}: {first[1]} iterations, residual {first[2]:.3e}")


@pytest.mark.parametrize("model,config", MODELS)
def test_fp32_ends_converged_or_stalled_with_a_finite_field(gpu, model, config):
    m = _ring_model(model, config, 256, 256, "f32")
    r0 = m.residual()["l2"]
    out = m.solve(1e-5 * r0, 20000)
    print(f"{model.__name__} fp32 256x256: {out['iterations']} iterations, {out['restarts']} restarts, residual "
          f"{out['residual']:.3e} (tol {1e-5 * r0:.3e}), {out['reason']}")
    assert out["reason"].startswith("converged") or out["reason"] == "stalled"
    assert bool(torch.isfinite(m.full()).all())


# -------------------------------------------------------------- errors, CLI
def test_errors_on_the_device(gpu):
    for solver in (hip().CgSolver, hip().PcgSolver):
        with pytest.raises(ValueError, match="singular.*Hold one side fixed.*screened"):
            solver(128, 128, "f64", 0.2, 0.2, neumann=list(ALL))
        with pytest.raises(ValueError, match="unknown side"):
            solver(128, 128, "f64", 0.2, 0.2, neumann=["north"])
        solver(128, 128, "f64", 0.19, 0.2, neumann=list(ALL))
    for config in (CgConfig, PcgConfig):
        with pytest.raises(ValueError, match="singular"):
            config(width=128, height=128, neumann=ALL)
        with pytest.raises(ValueError, match="unknown side"):
            config(width=128, height=128, neumann=("north",))


def test_cli_solves_with_insulated_walls(gpu, tmp_path):
    path = tmp_path / "pcg.json"
    cmd = [sys.executable, "-m", "cuda_mpi_scratch_amd.models.pcg2d", "--size", "256x256", "--dtype", "f64",
           "--source", "1e-6", "--tol", "1e-8", "--neumann", "left,right", "--json", str(path)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    rec = json.loads(path.read_text().splitlines()[-1])
    assert rec["metric"] == "pcg2d_solve_s" and rec["converged"] and rec["residual"] <= 1e-8
    assert rec["neumann"] == ["left", "right"] and rec["config"]["neumann"] == ["left", "right"]
    assert 0 < rec["iterations"] <= 40 and rec["graph"] == "captured" and rec["device"].startswith("cuda")
    assert "Neumann sides left, right" in rec["note"]
