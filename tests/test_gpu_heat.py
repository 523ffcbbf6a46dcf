"""Implicit heat steps on the GPU: the fused start kernels bit for bit against
``heat_start_reference`` (and what they may read and write) on the shape edges
tests/test_gpu_cg.py documents, under every Neumann side set, against the
unfused ``cg_start`` / ``pcg_start`` on the stored right-hand side, on unaligned
tiles, their refusals; and the native ``step()``: against the fp64 CPU twin, the
amplification of a sine mode, independent of the check cadence and of the
graph, its refusal of foreign weights, its residual, and the CLI."""
import json
import math
import os
import subprocess
import sys

import pytest
import torch

from cuda_mpi_scratch_amd import core, hip, ops
from cuda_mpi_scratch_amd.models import HeatConfig, ImplicitHeat2D
from tests.test_gpu_cg import _fields, _same_bits, _sum_check
from tests.test_gpu_multigrid import DT, SENTINEL, _assert_only_core_written, _core, _geom, _rand, _tile
from tests.test_heat_cpu import NEUMANN_SETS, amplification_check

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CACHE = {}
LAM = 3.0
# The edges of tests/test_gpu_cg.py's SHAPES: narrower than a 16-byte vector; an
# odd width with a ragged last vector; a second wave strip (fp64) and a ragged
# last band; several strips, an odd width and a 3-row last band; several
# workgroups across with a 1-row last band; more 4-row chunks than workgroups.
SHAPES = [(3, 3), (7, 5), (130, 70), (259, 131), (2051, 9), (5, 2090)]
EPS32 = 2.0 ** -24


def _inputs(w, h, dt):
    """u with NaN ring corners (no kernel may read them) and q, on the CPU."""
    key = ("inputs", w, h, dt)
    if key not in _CACHE:
        f = _fields(w, h, dt)
        u = f["u"].clone()
        u[0, 0] = u[0, -1] = u[-1, 0] = u[-1, -1] = float("nan")
        _CACHE[key] = (u, (f["q"] * 0.25).to(dt))
    return _CACHE[key]


def _reference(w, h, dtype, theta, with_q, neumann=()):
    key = ("start", w, h, dtype, theta, with_q, neumann)
    if key not in _CACHE:
        u, q = _inputs(w, h, DT[dtype])
        _CACHE[key] = ops.heat_start_reference(u, q if with_q else None, LAM, theta, neumann)
    return _CACHE[key]


def _run_both(gpu, g, dt, u_full, q_core, theta, neumann, check):
    """cg_heat_start and pcg_heat_start on fresh tiles: u and q with NaN wherever
    no kernel may read, the outputs pre-filled with the sentinel.
    check(name, tiles: dict, scalars: dict, ws)."""
    for name in ("cg_heat_start", "pcg_heat_start"):
        u = _tile(gpu, g, dt, full=u_full)                                  # padding and corners NaN
        q = None if q_core is None else _tile(gpu, g, dt, core_vals=q_core)  # ring and padding NaN
        out = {k: _tile(gpu, g, dt, fill=SENTINEL) for k in (("g", "r", "p") if name == "cg_heat_start" else ("g", "r"))}
        u0, q0 = u.clone(), None if q is None else q.clone()
        ws = (ops.CgWorkspace if name == "cg_heat_start" else ops.PcgWorkspace)(g, gpu)
        ws.write(tol=0.0, max_iters=9, norm="l2", iteration=5, beta=3.0, alpha=2.0, pq=1.0, status=2)
        if name == "cg_heat_start":
            ops.cg_heat_start(u, q, out["g"], out["r"], out["p"], g, LAM, theta, ws, neumann=neumann)
        else:
            ops.pcg_heat_start(u, q, out["g"], out["r"], g, LAM, theta, ws, neumann=neumann)
        torch.cuda.synchronize()
        assert hip().last_cg_dispatch() == name
        assert _same_bits(u, u0) and (q is None or _same_bits(q, q0)), f"{name} changed u or q"
        check(name, out, ws.read(), ws)


def _check_against(want, g, what):
    want_g, want_r, _, linf = want

    def check(name, out, sc, ws):
        _assert_only_core_written(out["g"], g, want_g, f"{name} g {what}")
        _assert_only_core_written(out["r"], g, want_r, f"{name} r {what}")
        if "p" in out:
            _assert_only_core_written(out["p"], g, want_r, f"{name} p {what}")
        _sum_check(f"{name} rr {what}", sc["rr"], want_r.double() ** 2)
        assert sc["linf"] == linf
        assert (sc["beta"], sc["alpha"], sc["pq"], sc["iteration"], sc["status"], sc["max_iters"], sc["tol"]) == \
            (0.0, 0.0, 0.0, 0, 0, 9, 0.0)
        assert sc.get("rz", 0.0) == 0.0
        assert int(ws.counter.item()) == 0, "the ticket was not put back"

    return check


# -------------------------------------------------------------------- kernels
@pytest.mark.parametrize("with_q", [False, True])
@pytest.mark.parametrize("theta", [1.0, 0.5])
@pytest.mark.parametrize("w,h", SHAPES)
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_heat_start_is_bitwise_the_reference(gpu, dtype, w, h, theta, with_q):
    """The gate: g, r and (CG) p of the fused kernel equal the reference bit for bit."""
    dt = DT[dtype]
    u, q = _inputs(w, h, dt)
    want = _reference(w, h, dtype, theta, with_q)
    g = _geom(w, h, dt)
    _run_both(gpu, g, dt, u, q if with_q else None, theta, (),
              _check_against(want, g, f"{dtype} {w}x{h} theta {theta} q {with_q}"))


@pytest.mark.parametrize("neumann", NEUMANN_SETS, ids=lambda n: "+".join(n) or "none")
@pytest.mark.parametrize("w,h", [(7, 5), (130, 70)])
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_heat_start_under_every_side_set(gpu, dtype, w, h, neumann):
    """Crank-Nicolson with a source; the ring of a Neumann side holds non-zero
    differences (the random ring), read as edge + ring in both parts."""
    dt = DT[dtype]
    u, q = _inputs(w, h, dt)
    want = _reference(w, h, dtype, 0.5, True, neumann)
    if not neumann:
        assert torch.equal(want[1], ops.heat_start_reference(u, q, LAM, 0.5)[1])
    else:
        assert not torch.equal(want[0], _reference(w, h, dtype, 0.5, True)[0])
    g = _geom(w, h, dt)
    _run_both(gpu, g, dt, u, q, 0.5, neumann, _check_against(want, g, f"{dtype} {w}x{h} {neumann}"))


@pytest.mark.parametrize("neumann", [(), ("bottom", "left")], ids=["dirichlet", "neumann"])
@pytest.mark.parametrize("w,h", [(259, 131), (2051, 9)])
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_fused_start_equals_the_unfused_start_on_the_stored_g(gpu, dtype, w, h, neumann):
    """cg_start / pcg_start with weights (0, c1) on (u, the g the fused kernel
    stored): the same bits in r, and rr and linf equal as doubles (the same grid
    and the same order of the partials)."""
    dt = DT[dtype]
    u_full, q_core = _inputs(w, h, dt)
    g = _geom(w, h, dt)
    c1 = ops.heat_coefficients(LAM, 0.5)["c1"]
    u, q = _tile(gpu, g, dt, full=u_full), _tile(gpu, g, dt, core_vals=q_core)
    for name in ("cg", "pcg"):
        ws = (ops.CgWorkspace if name == "cg" else ops.PcgWorkspace)(g, gpu)
        ws.write(tol=0.0, max_iters=9, norm="l2")
        gt = _tile(gpu, g, dt)  # ring and padding NaN: the unfused start may read the core of g only
        r1, p1, r2, p2 = (_tile(gpu, g, dt, fill=SENTINEL) for _ in range(4))
        if name == "cg":
            ops.cg_heat_start(u, q, gt, r1, p1, g, LAM, 0.5, ws, neumann=neumann)
        else:
            ops.pcg_heat_start(u, q, gt, r1, g, LAM, 0.5, ws, neumann=neumann)
        fused = ws.read()
        ws.write(rr=-1.0, linf=-1.0, status=3)
        if name == "cg":
            ops.cg_start(u, gt, r2, p2, g, 0.0, c1, ws, neumann=neumann)
        else:
            ops.pcg_start(u, gt, r2, g, 0.0, c1, ws, neumann=neumann)
        unfused = ws.read()
        assert bool(torch.isfinite(_core(gt, g)).all()) and bool(torch.isfinite(_core(r1, g)).all())
        assert _same_bits(r1, r2) and _same_bits(p1, p2), f"{name}: the fused residual is not the unfused one"
        print(f"{name} {dtype} {w}x{h} {neumann}: rr fused {fused['rr']!r}, unfused {unfused['rr']!r}")
        assert fused["rr"] == unfused["rr"] > 0 and fused["linf"] == unfused["linf"] > 0
        assert fused["status"] == unfused["status"] == 0


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_unaligned_tiles_take_the_guarded_path(gpu, dtype):
    """A compact tile (pitch = width + 2, the core one element into each row) is
    not 16-byte aligned: every load and store goes element by element."""
    dt = DT[dtype]
    w, h = 130, 70
    u, q = _inputs(w, h, dt)
    g = core().TileGeom.compact(w, h, 1, 1)
    for with_q, neumann in ((True, ()), (False, ("top", "right"))):
        want = _reference(w, h, dtype, 0.5, with_q, neumann)
        _run_both(gpu, g, dt, u, q if with_q else None, 0.5, neumann,
                  _check_against(want, g, f"{dtype} compact q {with_q} {neumann}"))


def test_launchers_refuse_bad_arguments(gpu):
    dt = torch.float64
    w, h = 64, 32
    g = _geom(w, h, dt)
    a, b, c, d, e = (_tile(gpu, g, dt, fill=0.0) for _ in range(5))
    ws, pws = ops.CgWorkspace(g, gpu), ops.PcgWorkspace(g, gpu)
    bare = core().TileGeom.aligned(w, h, 0, 0, 8)
    with pytest.raises(Exception, match="cg_heat_start.*no ghost ring"):
        ops.cg_heat_start(a, None, b, c, d, bare, LAM, 1.0, ws)
    with pytest.raises(Exception, match="pcg_heat_start.*no ghost ring"):
        ops.pcg_heat_start(a, e, b, c, bare, LAM, 1.0, pws)
    with pytest.raises(Exception, match="four tiles"):
        ops.cg_heat_start(a, None, b, c, c, g, LAM, 1.0, ws)   # r == p
    with pytest.raises(Exception, match="four tiles"):
        ops.cg_heat_start(a, None, a, c, d, g, LAM, 1.0, ws)   # g == u
    with pytest.raises(Exception, match="three tiles"):
        ops.pcg_heat_start(a, None, b, b, g, LAM, 1.0, pws)    # g == r
    with pytest.raises(Exception, match="source q must not be one of the written tiles"):
        ops.cg_heat_start(a, b, b, c, d, g, LAM, 1.0, ws)      # q == g
    with pytest.raises(Exception, match="source q must not be one of the written tiles"):
        ops.pcg_heat_start(a, c, b, c, g, LAM, 1.0, pws)       # q == r
    with pytest.raises(Exception, match="needs every tile"):
        hip().cg_heat_start(0, 0, b.data_ptr(), c.data_ptr(), d.data_ptr(), g, LAM, 1.0, *ws._ptrs(), "f64")
    with pytest.raises(Exception, match="needs every tile"):
        hip().pcg_heat_start(a.data_ptr(), 0, 0, c.data_ptr(), g, LAM, 1.0, *pws._ptrs(), "f64")
    with pytest.raises(Exception, match="scalar block"):
        hip().cg_heat_start(a.data_ptr(), 0, b.data_ptr(), c.data_ptr(), d.data_ptr(), g, LAM, 1.0, 0, 0, 0, "f64")
    host = torch.zeros(g.alloc_elems(), dtype=dt)
    with pytest.raises(TypeError, match="GPU tensors only"):
        ops.cg_heat_start(a, host, b, c, d, g, LAM, 1.0, ws)
    with pytest.raises(TypeError, match="GPU tensors only"):
        ops.pcg_heat_start(host, None, b, c, g, LAM, 1.0, pws)
    with pytest.raises(ValueError, match="conditionally stable"):
        ops.cg_heat_start(a, None, b, c, d, g, LAM, 0.3, ws)
    with pytest.raises(ValueError, match="unknown side"):
        ops.cg_heat_start(a, None, b, c, d, g, LAM, 1.0, ws, neumann=("north",))
    torch.cuda.synchronize()


# --------------------------------------------------------------------- solver
NEUMANN_PAIR = ("left", "right")


def _heat_problem(w, h, dtype, device, lam, theta, method, **kw):
    """Dirichlet values top and bottom, prescribed differences on the Neumann
    pair, a random start and a random source; fp64 data on every backend."""
    m = ImplicitHeat2D(HeatConfig(width=w, height=h, dtype=dtype, lam=lam, theta=theta, method=method,
                                  neumann=NEUMANN_PAIR, **kw), device=device)
    gen = torch.Generator(device="cpu").manual_seed(w + 3 * h)
    m.set_boundary(top=1.0, bottom=_rand((w,), gen, torch.float64), left=_rand((h,), gen, torch.float64, 0.05), right=0.02)
    m.set_field(_rand((h, w), gen, torch.float64))
    m.set_source(_rand((h, w), gen, torch.float64, 0.1))
    return m


def _twin(lam, theta, method, tol, n):
    key = ("twin", lam, theta, method, tol, n)
    if key not in _CACHE:
        ref = _heat_problem(130, 70, "f64", "cpu", lam, theta, method)
        start = ref.full()
        steps = [ref.step(1, tol) for _ in range(n)]
        _CACHE[key] = (start, steps, ref.field())
    return _CACHE[key]


@pytest.mark.parametrize("method", ["pcg", "cg"])
@pytest.mark.parametrize("lam", [0.2, 200.0])
@pytest.mark.parametrize("theta", [1.0, 0.5])
def test_step_against_the_cpu_twin(gpu, theta, lam, method):
    """Both sides solve every step to tol, so each is within D tol of the exact
    step of its own previous field; the step map is a contraction in l2, so the
    two fields part by at most 2 D tol per step: ||u_gpu - u_twin||_2 <= 2 n D tol."""
    w, h, n, tol = 130, 70, 3, 1e-9
    D = 1 + 4 * theta * lam
    start, steps, u_twin = _twin(lam, theta, method, tol, n)
    assert all(s["converged"] for s in steps), steps
    m = _heat_problem(w, h, "f64", "cuda", lam, theta, method)
    assert m.solver is not None
    assert torch.equal(m.full().cpu(), start), "set_boundary / set_field differ between the backends"
    for k, s in enumerate(steps):
        out = m.step(1, tol, max_iters=2 * s["iterations"][0])
        print(f"{method} lam {lam} theta {theta} step {k + 1}: device {out['iterations']} iterations "
              f"({out['restarts']} restarts), twin {s['iterations']} ({s['restarts']}), residual {out['residuals']}")
        assert out["converged"], out
        assert out["iterations"][0] <= 2 * s["iterations"][0]
    diff = float(torch.linalg.vector_norm(m.field().cpu() - u_twin))
    bound = 2 * n * D * tol * (1 + 1e-6)
    print(f"{method} lam {lam} theta {theta}: ||u_gpu - u_twin||_2 {diff:.3e}, bound {bound:.3e}")
    assert diff <= bound
    assert m.time_steps_total == n


def test_fp32_step_against_the_fp64_twin(gpu):
    """The bound of test_step_against_the_cpu_twin plus the fp32 run's own
    roundings of the right-hand side, 12 n D eps32 ||u0||_2: per cell and step,
    relative to |u| (|a| <= 1, 4 b < 1, 4 c1 < 1, |g| <~ |u|), one rounding each
    for the stored field, the coefficients a, b, s and c1 (the last perturbs the
    operator by eps32 c1 S), the product a c, the fma, the product s q and the
    last sum, and three for the sum S weighted by b: 12 eps32 |u|, which the
    inverse of L (norm <= D) amplifies by at most D."""
    w, h, n, lam, theta = 130, 70, 3, 2.0, 0.5
    D = 1 + 4 * theta * lam
    ref = _heat_problem(w, h, "f64", "cpu", lam, theta, "pcg")
    norm0 = float(torch.linalg.vector_norm(ref.field()))
    tol = 1e-5 * norm0
    assert ref.step(n, tol)["converged"]
    m = _heat_problem(w, h, "f32", "cuda", lam, theta, "pcg")
    out = m.step(n, tol)
    diff = float(torch.linalg.vector_norm(m.field().cpu().double() - ref.field()))
    bound = 2 * n * D * tol * (1 + 1e-6) + 12 * n * D * EPS32 * norm0
    print(f"fp32 pcg lam {lam}: iterations {out['iterations']}, restarts {out['restarts']}, ||u_gpu - u_twin||_2 "
          f"{diff:.3e}, bound {bound:.3e}")
    assert out["converged"] and out["steps"] == n, out
    assert diff <= bound


@pytest.mark.parametrize("w,h,method", [(33, 21, "cg"), (130, 70, "pcg")])
@pytest.mark.parametrize("lam", [0.2, 50.0, 1e4])
@pytest.mark.parametrize("theta", [1.0, 0.5])
def test_amplification_of_a_sine_mode_on_the_device(gpu, theta, lam, w, h, method):
    def make():
        m = ImplicitHeat2D(HeatConfig(width=w, height=h, dtype="f64", lam=lam, theta=theta, method=method), device="cuda")
        assert m.solver is not None
        return m

    amplification_check(make, w, h, lam, theta)


@pytest.mark.parametrize("method", ["pcg", "cg"])
def test_the_cadence_and_the_graph_change_no_bit(gpu, method):
    first = None
    for graph in (True, False):
        for every in (1, 2, 16):
            m = _heat_problem(130, 70, "f64", "cuda", 50.0, 0.5, method, graph=graph, check_every=every)
            out = m.step(3, 1e-9)
            got = m.full()
            print(f"{method} check_every {every}, graph {graph} ({m.graph_status()}): iterations {out['iterations']}, "
                  f"residuals {out['residuals']}")
            assert out["converged"] and out["steps"] == 3, out
            assert m.graph_status() == ("captured" if graph else "off")
            if first is None:
                first = (got, out["iterations"], out["residuals"], out["restarts"])
            assert _same_bits(got, first[0]), "the field depends on the cadence or on the graph"
            assert (out["iterations"], out["residuals"], out["restarts"]) == first[1:]


def test_step_refuses_foreign_weights(gpu):
    c1 = ops.heat_coefficients(2.0, 1.0)["c1"]
    for solver in (hip().CgSolver(64, 32, "f64", 0.2, 0.2), hip().PcgSolver(64, 32, "f64", 0.0, 0.2),
                   hip().CgSolver(64, 32, "f64", 1e-3, c1)):
        with pytest.raises(ValueError, match="step\\(\\) needs a solver built with.*\\(0, 0.2222222222222222.\\).*this one has"):
            solver.step(2.0, 1.0, 1e-8)
    ok = hip().CgSolver(64, 32, "f64", 0.0, c1)
    assert ok.step(2.0, 1.0, 1e-8)["converged"]
    with pytest.raises(ValueError, match="step\\(\\) needs"):
        ok.step(2.0, 0.5, 1e-8)
    with pytest.raises(ValueError, match="norm"):
        ok.step(2.0, 1.0, 1e-8, 5, "l1")
    with pytest.raises(ValueError, match="conditionally stable"):
        ok.step(2.0, 0.1, 1e-8)


@pytest.mark.parametrize("neumann", [(), ("top",)], ids=["dirichlet", "neumann"])
@pytest.mark.parametrize("method", ["pcg", "cg"])
def test_residual_after_a_step_and_a_source_taken_away(gpu, method, neumann):
    """residual() after a step is that step's true residual: the stored g is the
    step's right-hand side. set_source(None) goes back to the no-source kernel."""
    w, h, lam, theta, tol = 96, 40, 10.0, 0.5, 1e-10
    c1 = ops.heat_coefficients(lam, theta)["c1"]
    gen = torch.Generator(device="cpu").manual_seed(77)
    u0, q = _rand((h, w), gen, torch.float64), _rand((h, w), gen, torch.float64, 0.1)
    m = ImplicitHeat2D(HeatConfig(width=w, height=h, lam=lam, theta=theta, method=method, neumann=neumann), device="cuda")
    m.set_boundary(top=0.1, left=0.5)
    m.set_field(u0)
    for src in (q, None):
        m.set_source(src)
        before = m.full().cpu()
        out = m.step(1, tol)
        after = m.full().cpu()
        g = ops.heat_rhs_reference(before, src, lam, theta, neumann)
        _, l2 = ops.residual5_reference(ops.ghosted(after, neumann), 1, 0.0, c1, source=g)
        res = m.residual()
        print(f"{method} {neumann} source {src is not None}: step residual {out['residuals'][0]:.3e}, residual() "
              f"{res['l2']:.3e}, recomputed {l2:.3e}")
        assert out["converged"] and out["residuals"][0] == res["l2"] <= tol
        # the two evaluations of a residual near 1e-10 may round each cell differently: 4 roundings of
        # values below 2 per cell at the most, over sqrt(N) in l2
        assert abs(res["l2"] - l2) <= 8 * math.sqrt(w * h) * 2.0 ** -53


def test_cli_steps_and_writes_its_json(gpu, tmp_path):
    path = tmp_path / "heat.json"
    cmd = [sys.executable, "-m", "cuda_mpi_scratch_amd.models.heat2d", "--size", "256x256", "--lam", "100", "--theta", "1",
           "--steps", "3", "--tol", "1e-10", "--source", "1e-3", "--neumann", "left,right", "--json", str(path)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    rec = json.loads(path.read_text().splitlines()[-1])
    assert rec == json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert rec["metric"] == "heat2d_step_s" and rec["value"] > 0 and rec["converged"] and rec["steps"] == 3
    assert len(rec["iterations"]) == 3 and all(0 < i <= 1000 for i in rec["iterations"])
    assert all(x <= 1e-10 for x in rec["residuals"]) and rec["reason"].startswith("converged")
    assert rec["graph"] == "captured" and rec["config"]["lam"] == 100 and rec["config"]["method"] == "pcg"
    assert rec["neumann"] == ["left", "right"] and rec["device"].startswith("cuda")
    assert "D = 1 + 4 theta lam = 401" in rec["note"] and "error per step <= D tol in l2" in rec["note"]
    assert math.isfinite(rec["total_s"]) and rec["time_steps_total"] == 3
