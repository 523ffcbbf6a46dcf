"""Conjugate gradients on the GPU: each of the three HIP kernels bit for bit
against its pure-torch reference (and what it may read and write), their fused
sums against the worst-case bound of a double summation, the status protocol,
the launchers' refusals, and the native solver: against a dense direct solve,
against the CPU twin, independent of the host's check cadence, on the grids and
operators multigrid refuses, its residual, fp32, the errors and the CLI."""
import json
import math
import os
import subprocess
import sys

import pytest
import torch

from cuda_mpi_scratch_amd import core, hip, ops
from cuda_mpi_scratch_amd.models.cg2d import CgConfig, ConjugateGradient2D
from cuda_mpi_scratch_amd.models.multigrid2d import Multigrid2D, MultigridConfig
from tests.relaxation_worker import BOUNDARY
from tests.test_cg_cpu import direct_solution, ring_problem, setup
from tests.test_gpu_multigrid import DT, SENTINEL, _assert_only_core_written, _core, _geom, _rand, _tile
from tests.test_source_cpu import manufactured

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CACHE = {}
WEIGHTS = [(0.2, 0.2), (0.5, 0.1)]
# A workgroup is four waves side by side, each a strip of 64 16-byte vectors:
# 1024 fp32 / 512 fp64 columns, walking a band of rows that is a multiple of 4:
# 4 rows while the launch has at most one workgroup per CU (256 on a whole
# MI355X), as for every shape here but the last. (3, 3) and (7, 5) sit inside
# one workgroup tile, narrower than a 16-byte vector (fp32) or with an odd width
# and a ragged last vector; (64, 32) is whole vectors only, 8 bands; (130, 70)
# has a ragged last band (2 rows) and, in fp64, a second wave strip with 2
# columns; (259, 131) has an odd width, 2 (fp32) or 3 (fp64) wave strips and a
# ragged last band (3 rows); (256, 96) is exactly one fp32 strip and two fp64
# strips of whole vectors. None of these is wider than one workgroup, so
# (2051, 9) is added: 3 (fp32) or 5 (fp64) workgroups across, the last with 3
# ragged columns, and 3 bands, the last with 1 row. (5, 2090) has more 4-row
# chunks (523) than a whole MI355X gets workgroups: 175 bands of 3 chunks, which
# roll the three-row window across chunk ends, the last band with 2 rows.
SHAPES = [(3, 3), (7, 5), (64, 32), (130, 70), (259, 131), (256, 96), (2051, 9), (5, 2090)]


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _fields(w, h, dtype):
    """Per shape and type, made once and left unchanged, on the CPU: u (core and
    ring), g, r, p, q (core sized)."""
    key = ("fields", w, h, dtype)
    if key not in _CACHE:
        gen = torch.Generator(device="cpu").manual_seed(1000 * w + h)
        _CACHE[key] = {"u": _rand((h + 2, w + 2), gen, dtype), "g": _rand((h, w), gen, dtype, 0.1),
                       "r": _rand((h, w), gen, dtype, 0.3), "p": _rand((h, w), gen, dtype),
                       "q": _rand((h, w), gen, dtype)}
    return _CACHE[key]


def _sum_check(what, have, terms):
    """|sum_device - sum_reference| <= (N + 1) 2^-53 sum |terms|: the worst case of
    any summation order of N double terms (the reference is their exact sum,
    rounded once)."""
    t = terms.double().reshape(-1).tolist()
    want, scale = math.fsum(t), math.fsum(abs(v) for v in t)
    bound = (len(t) + 1) * 2.0 ** -53 * scale
    print(f"{what}: device {have!r}, reference {want!r}, |difference| {abs(have - want):.3e}, bound {bound:.3e}")
    assert abs(have - want) <= bound


# -------------------------------------------------------------------- kernels
@pytest.mark.parametrize("w,h", SHAPES)
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_start_is_bitwise_the_reference(gpu, dtype, w, h):
    dt = DT[dtype]
    f = _fields(w, h, dt)
    c0, c1 = 0.5, 0.1
    key = ("start", w, h, dtype)
    if key not in _CACHE:
        _CACHE[key] = ops.cg_start_reference(f["u"], f["g"], c0, c1)
    want, _, linf = _CACHE[key]
    g = _geom(w, h, dt)
    u = _tile(gpu, g, dt, full=f["u"])          # padding NaN: only core and ring may be read
    src = _tile(gpu, g, dt, core_vals=f["g"])   # ring and padding NaN
    r, p = _tile(gpu, g, dt, fill=SENTINEL), _tile(gpu, g, dt, fill=SENTINEL)
    u0, src0 = u.clone(), src.clone()
    ws = ops.CgWorkspace(g, gpu)
    ws.write(tol=0.0, max_iters=9, norm="l2", iteration=5, beta=3.0, status=2)
    ops.cg_start(u, src, r, p, g, c0, c1, ws)
    torch.cuda.synchronize()
    assert hip().last_cg_dispatch() == "cg_start"
    _assert_only_core_written(r, g, want, f"cg_start r {dtype} {w}x{h}")
    _assert_only_core_written(p, g, want, f"cg_start p {dtype} {w}x{h}")
    assert _same_bits(u, u0) and _same_bits(src, src0), "cg_start changed u or g"
    sc = ws.read()
    _sum_check(f"cg_start rr {dtype} {w}x{h}", sc["rr"], want.double() ** 2)
    assert sc["linf"] == linf
    assert (sc["beta"], sc["iteration"], sc["status"], sc["max_iters"], sc["tol"]) == (0.0, 0, 0, 9, 0.0)
    assert int(ws.counter.item()) == 0, "the ticket was not put back"


@pytest.mark.parametrize("beta", [0.0, 0.37])
@pytest.mark.parametrize("w,h", SHAPES)
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_apply_is_bitwise_the_reference(gpu, dtype, w, h, beta):
    dt = DT[dtype]
    f = _fields(w, h, dt)
    c0, c1 = 0.5, 0.1
    key = ("apply", w, h, dtype, beta)
    if key not in _CACHE:
        _CACHE[key] = ops.cg_apply_reference(f["r"], f["p"], beta, c0, c1)
    want_p, want_q, _ = _CACHE[key]
    g = _geom(w, h, dt)
    r, p_old = _tile(gpu, g, dt, core_vals=f["r"]), _tile(gpu, g, dt, core_vals=f["p"])  # ring and padding NaN
    p_new, q = _tile(gpu, g, dt, fill=SENTINEL), _tile(gpu, g, dt, fill=SENTINEL)
    r0, p0 = r.clone(), p_old.clone()
    ws = ops.CgWorkspace(g, gpu)
    rr = 1.25
    ws.write(beta=beta, rr=rr, tol=0.0, max_iters=100, iteration=3)
    ops.cg_apply(r, p_old, p_new, q, g, c0, c1, ws)
    torch.cuda.synchronize()
    assert hip().last_cg_dispatch() == "cg_apply"
    _assert_only_core_written(p_new, g, want_p, f"cg_apply p_new {dtype} {w}x{h} beta={beta}")
    _assert_only_core_written(q, g, want_q, f"cg_apply q {dtype} {w}x{h} beta={beta}")
    assert _same_bits(r, r0) and _same_bits(p_old, p0), "cg_apply changed r or p_old"
    sc = ws.read()
    _sum_check(f"cg_apply pq {dtype} {w}x{h}", sc["pq"], want_p.double() * want_q.double())
    assert sc["pq"] > 0 and sc["alpha"] == rr / sc["pq"], "alpha is not the double quotient of the stored rr and pq"
    assert (sc["status"], sc["iteration"], sc["rr"], sc["beta"]) == (0, 3, rr, beta)
    assert int(ws.counter.item()) == 0


@pytest.mark.parametrize("w,h", SHAPES)
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_update_is_bitwise_the_reference(gpu, dtype, w, h):
    dt = DT[dtype]
    f = _fields(w, h, dt)
    alpha, rr_old = 0.61, 2.5
    key = ("update", w, h, dtype)
    if key not in _CACHE:
        _CACHE[key] = ops.cg_update_reference(f["u"][1:-1, 1:-1], f["r"], f["p"], f["q"], alpha)
    want_u, want_r, _, linf = _CACHE[key]
    g = _geom(w, h, dt)
    # in place: the ring and the padding of u and r hold the sentinel, those of p and q NaN
    u = _tile(gpu, g, dt, core_vals=f["u"][1:-1, 1:-1], fill=SENTINEL)
    r = _tile(gpu, g, dt, core_vals=f["r"], fill=SENTINEL)
    p, q = _tile(gpu, g, dt, core_vals=f["p"]), _tile(gpu, g, dt, core_vals=f["q"])
    p0, q0 = p.clone(), q.clone()
    ws = ops.CgWorkspace(g, gpu)
    ws.write(alpha=alpha, rr=rr_old, tol=0.0, max_iters=100, iteration=4, norm="linf")
    ops.cg_update(u, r, p, q, g, ws)
    torch.cuda.synchronize()
    assert hip().last_cg_dispatch() == "cg_update"
    _assert_only_core_written(u, g, want_u, f"cg_update u {dtype} {w}x{h}")
    _assert_only_core_written(r, g, want_r, f"cg_update r {dtype} {w}x{h}")
    assert _same_bits(p, p0) and _same_bits(q, q0), "cg_update changed p or q"
    sc = ws.read()
    _sum_check(f"cg_update rr {dtype} {w}x{h}", sc["rr"], want_r.double() ** 2)
    assert sc["linf"] == linf
    assert sc["beta"] == sc["rr"] / rr_old, "beta is not the double quotient of the new and the old rr"
    assert (sc["iteration"], sc["status"], sc["alpha"]) == (5, 0, alpha)
    assert int(ws.counter.item()) == 0


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_unaligned_tiles_take_the_guarded_path(gpu, dtype):
    """A compact tile (pitch = width + 2, the core one element into each row) is
    not 16-byte aligned: every load and store goes element by element."""
    dt = DT[dtype]
    w, h = 130, 70
    f = _fields(w, h, dt)
    g = core().TileGeom.compact(w, h, 1, 1)
    want_p, want_q, _ = ops.cg_apply_reference(f["r"], f["p"], 0.37, 0.2, 0.2)
    r, p_old = _tile(gpu, g, dt, core_vals=f["r"]), _tile(gpu, g, dt, core_vals=f["p"])
    p_new, q = _tile(gpu, g, dt, fill=SENTINEL), _tile(gpu, g, dt, fill=SENTINEL)
    ws = ops.CgWorkspace(g, gpu)
    ws.write(beta=0.37, rr=1.0, max_iters=10)
    ops.cg_apply(r, p_old, p_new, q, g, 0.2, 0.2, ws)
    _assert_only_core_written(p_new, g, want_p, f"cg_apply p_new {dtype} compact")
    _assert_only_core_written(q, g, want_q, f"cg_apply q {dtype} compact")
    want_r, _, _ = ops.cg_start_reference(f["u"], f["g"], 0.2, 0.2)
    u, src = _tile(gpu, g, dt, full=f["u"]), _tile(gpu, g, dt, core_vals=f["g"])
    r2, p2 = _tile(gpu, g, dt, fill=SENTINEL), _tile(gpu, g, dt, fill=SENTINEL)
    ops.cg_start(u, src, r2, p2, g, 0.2, 0.2, ws)
    _assert_only_core_written(r2, g, want_r, f"cg_start r {dtype} compact")
    want_u, want_r1, _, _ = ops.cg_update_reference(f["u"][1:-1, 1:-1], want_r, want_p, want_q, 0.61)
    ws.write(alpha=0.61, status=0, max_iters=10)
    uu = _tile(gpu, g, dt, core_vals=f["u"][1:-1, 1:-1], fill=SENTINEL)
    ops.cg_update(uu, r2, p_new, q, g, ws)
    _assert_only_core_written(uu, g, want_u, f"cg_update u {dtype} compact")
    _assert_only_core_written(r2, g, want_r1, f"cg_update r {dtype} compact")


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_status_protocol(gpu, dtype):
    dt = DT[dtype]
    w, h = 130, 70
    f = _fields(w, h, dt)
    g = _geom(w, h, dt)
    c0, c1 = 0.2, 0.2
    ws = ops.CgWorkspace(g, gpu)
    u, src = _tile(gpu, g, dt, full=f["u"]), _tile(gpu, g, dt, core_vals=f["g"])
    r, p = _tile(gpu, g, dt, fill=SENTINEL), _tile(gpu, g, dt, fill=SENTINEL)
    p2, q = _tile(gpu, g, dt, fill=SENTINEL), _tile(gpu, g, dt, fill=SENTINEL)
    _, rr, linf = ops.cg_start_reference(f["u"], f["g"], c0, c1)
    # cg_start: a tolerance above the norm converges at once, in either norm; no iterations allowed is status 2
    for norm, tol, want in [("l2", 2 * math.sqrt(rr), 1), ("l2", 0.5 * math.sqrt(rr), 0), ("linf", 2 * linf, 1),
                            ("linf", 0.5 * linf, 0)]:
        ws.write(tol=tol, max_iters=10, norm=norm, status=0)
        ops.cg_start(u, src, r, p, g, c0, c1, ws)
        assert ws.read()["status"] == want, (norm, tol)
    ws.write(tol=0.0, max_iters=0, norm="l2")
    ops.cg_start(u, src, r, p, g, c0, c1, ws)
    assert ws.read()["status"] == 2
    # one iteration with max_iters = 1: status 2 and the counter 1; with a tolerance above the norm: status 1
    for tol, max_iters, want in [(0.0, 1, 2), (1e30, 1, 1), (1e30, 5, 1), (0.0, 5, 0)]:
        ws.write(tol=tol, max_iters=max_iters, norm="l2")
        ops.cg_start(u, src, r, p, g, c0, c1, ws)
        ws.write(status=0)
        ops.cg_apply(r, p, p2, q, g, c0, c1, ws)
        ops.cg_update(u.clone(), r.clone(), p2, q, g, ws)
        sc = ws.read()
        assert (sc["status"], sc["iteration"]) == (want, 1), (tol, max_iters, sc)
    # with a status != 0 at entry both kernels leave every tile bitwise unchanged, and the scalars too
    tiles = [u, r, p, p2, q]
    for status in (1, 2, 3):
        ws.write(status=status, alpha=0.5, beta=0.25)
        before, sc0 = [t.clone() for t in tiles], ws.read()
        ops.cg_apply(r, p, p2, q, g, c0, c1, ws)
        ops.cg_update(u, r, p2, q, g, ws)
        torch.cuda.synchronize()
        assert all(_same_bits(a, b) for a, b in zip(tiles, before)), f"status {status}: a tile changed"
        assert ws.read() == sc0 and int(ws.counter.item()) == 0
    # p = 0: pq = 0 is a breakdown, alpha = 0, and nothing is NaN
    zr, zp = _tile(gpu, g, dt, core_vals=torch.zeros(h, w, dtype=dt)), _tile(gpu, g, dt, core_vals=torch.zeros(h, w, dtype=dt))
    ws.write(status=0, beta=0.37, rr=1.0, alpha=9.0, max_iters=10)
    ops.cg_apply(zr, zp, p2, q, g, c0, c1, ws)
    sc = ws.read()
    assert (sc["status"], sc["alpha"], sc["pq"]) == (3, 0.0, 0.0)
    assert bool((_core(p2, g) == 0).all()) and bool((_core(q, g) == 0).all())


def test_launchers_refuse_bad_arguments(gpu):
    dt = torch.float64
    w, h = 64, 32
    g = _geom(w, h, dt)
    a, b, c, d = (_tile(gpu, g, dt, fill=0.0) for _ in range(4))
    ws = ops.CgWorkspace(g, gpu)
    bare = core().TileGeom.aligned(w, h, 0, 0, 8)
    with pytest.raises(Exception, match="no ghost ring"):
        ops.cg_start(a, b, c, d, bare, 0.2, 0.2, ws)
    with pytest.raises(Exception, match="no ghost ring"):
        ops.cg_apply(a, b, c, d, bare, 0.2, 0.2, ws)
    with pytest.raises(Exception, match="no ghost ring"):
        ops.cg_update(a, b, c, d, bare, ws)
    with pytest.raises(Exception, match="p_old != p_new"):
        ops.cg_apply(a, b, b, d, g, 0.2, 0.2, ws)
    with pytest.raises(Exception, match="four tiles"):
        ops.cg_update(a, a, c, d, g, ws)
    host = torch.zeros(g.alloc_elems(), dtype=dt)
    with pytest.raises(TypeError, match="GPU tensors only"):
        ops.cg_start(host, b, c, d, g, 0.2, 0.2, ws)
    with pytest.raises(TypeError, match="GPU tensors only"):
        ops.cg_apply(a, b, host, d, g, 0.2, 0.2, ws)
    with pytest.raises(TypeError, match="GPU tensors only"):
        ops.cg_update(a, b, c, host, g, ws)


# --------------------------------------------------------------------- solver
def _problem(w, h, dtype, device, **kw):
    """The data of test_gpu_multigrid._problem: non-zero boundaries on all sides,
    a random start and a random source."""
    m = ConjugateGradient2D(CgConfig(width=w, height=h, dtype=dtype, **kw), device=device)
    gen = torch.Generator(device="cpu").manual_seed(w + 3 * h)
    m.set_boundary(top=1.0, bottom=_rand((w,), gen, torch.float64), left=torch.linspace(1.0, 0.0, h, dtype=torch.float64),
                   right=-0.5)
    m.set_field(_rand((h, w), gen, torch.float64))
    m.set_source(_rand((h, w), gen, torch.float64, 1e-3))
    return m


@pytest.mark.parametrize("c0,c1", WEIGHTS)
def test_solver_against_the_dense_direct_solve(gpu, c0, c1):
    w, h, tol = 35, 19, 1e-10
    prob = ring_problem(w, h)
    m = ConjugateGradient2D(CgConfig(width=w, height=h, dtype="f64", c_center=c0, c_neighbor=c1), device="cuda")
    assert m.solver is not None
    setup(m, prob)
    out = m.solve(tol, 4 * w * h)
    a = ops.relaxation_spectrum(w, h, c0, c1)[0]
    err = float(torch.linalg.vector_norm(m.field().cpu() - direct_solution(w, h, c0, c1, prob)))
    print(f"device {w}x{h} ({c0}, {c1}): {out['iterations']} iterations, {out['restarts']} restarts, true l2 residual "
          f"{out['residual']:.3e}, ||u - u_direct||_2 {err:.3e}, bound {tol / a:.3e}")
    assert out["converged"] and out["residual"] <= tol, out["reason"]
    assert err <= (tol / a) * (1 + 1e-6)


def _twin_130x70():
    if "twin" not in _CACHE:
        ref = _problem(130, 70, "f64", "cpu")
        start, r0 = ref.full(), ref.residual()["l2"]
        out = ref.solve(1e-10 * r0, 20000)
        _CACHE["twin"] = (start, r0, out, ref.field())
    return _CACHE["twin"]


def test_solver_against_the_cpu_twin(gpu):
    """Both solve one problem to tol, so ||u_gpu - u_twin||_2 <= 2 tol / a; the
    device may take at most twice the twin's own iterations."""
    w, h = 130, 70
    start, r0, twin, u_twin = _twin_130x70()
    tol = 1e-10 * r0
    assert twin["converged"], twin["reason"]
    m = _problem(w, h, "f64", "cuda")
    assert torch.equal(m.full().cpu(), start), "set_boundary / set_field differ between the backends"
    assert m.residual()["l2"] == pytest.approx(r0, rel=1e-12)
    out = m.solve(tol, 2 * twin["iterations"])
    a = ops.relaxation_spectrum(w, h, 0.2, 0.2)[0]
    diff = float(torch.linalg.vector_norm(m.field().cpu() - u_twin))
    print(f"130x70 fp64: device {out['iterations']} iterations ({out['restarts']} restarts), twin {twin['iterations']} "
          f"({twin['restarts']} restarts); ||u_gpu - u_twin||_2 {diff:.3e}, bound {2 * tol / a:.3e}")
    assert out["converged"], out["reason"]
    assert out["iterations"] <= 2 * twin["iterations"]
    assert diff <= 2 * tol / a


def test_the_check_cadence_changes_no_bit(gpu):
    w, h = 130, 70
    _, r0, _, _ = _twin_130x70()
    tol = 1e-10 * r0
    first = None
    for graph in (True, False):
        for every in (1, 2, 16, 64):
            m = _problem(w, h, "f64", "cuda", graph=graph, check_every=every)
            out = m.solve(tol, 5000)
            got = m.full()
            print(f"check_every {every}, graph {graph} ({m.graph_status()}): {out['iterations']} iterations, "
                  f"{len(out['history'])} checks, residual {out['residual']:.3e}")
            assert out["converged"], out["reason"]
            assert m.graph_status() == ("captured" if graph else "off")
            if first is None:
                first = (got, out["iterations"], out["residual"], out["restarts"])
            assert _same_bits(got, first[0]), "the field depends on the cadence"
            assert (out["iterations"], out["residual"], out["restarts"]) == first[1:]


@pytest.mark.parametrize("graph", [True, False])
def test_exact_iteration_cap(gpu, graph):
    m = _problem(130, 70, "f64", "cuda", graph=graph)
    out = m.solve(0.0, 37)
    sc = m.scalars()
    print(f"cap 37, graph {graph}: {out['iterations']} iterations, reason {out['reason']!r}, device counter {sc['iteration']}")
    assert out["iterations"] == 37 and out["reason"] == "max_iters reached" and not out["converged"]
    assert sc["iteration"] == 37 and sc["status"] == 2 and sc["max_iters"] == 37


@pytest.mark.parametrize("w,h,c0,c1", [(128, 64, 0.5, 0.1), (2048, 16, 0.2, 0.2)])
def test_solves_what_multigrid_refuses(gpu, w, h, c0, c1):
    with pytest.raises(ValueError):
        Multigrid2D(MultigridConfig(width=w, height=h, c_center=c0, c_neighbor=c1), device="cuda")
    tol = 1e-9
    src = _rand((h, w), torch.Generator(device="cpu").manual_seed(w + h), torch.float64, 0.01)
    m = ConjugateGradient2D(CgConfig(width=w, height=h, dtype="f64", c_center=c0, c_neighbor=c1), device="cuda")
    m.set_boundary(**BOUNDARY)
    m.set_source(src)
    out = m.solve(tol, 4 * w * h)
    _, l2 = ops.residual5_reference(m.full().cpu(), 1, c0, c1, source=src)
    print(f"{w}x{h} ({c0}, {c1}): {out['iterations']} iterations, residual {out['residual']:.3e}, recomputed {l2:.3e}")
    assert out["converged"], out["reason"]
    assert l2 <= tol and out["residual"] == pytest.approx(l2, rel=1e-9)


def test_cross_check_against_multigrid(gpu):
    """Two independent solvers of one problem: ||u_cg - u_mg||_2 <= (||r_cg||_2 +
    ||r_mg||_2) / a <= 2 tol / a."""
    w, h, tol = 127, 63, 1e-10
    _, _, a = manufactured(w, h)
    src = _rand((h, w), torch.Generator(device="cpu").manual_seed(21), torch.float64, 0.01)
    sols = []
    for cls, cfg in ((ConjugateGradient2D, CgConfig(width=w, height=h, dtype="f64")),
                     (Multigrid2D, MultigridConfig(width=w, height=h, dtype="f64"))):
        m = cls(cfg, device="cuda")
        m.set_boundary(**BOUNDARY)
        m.set_source(src)
        out = m.solve(tol, 4 * w * h) if cls is ConjugateGradient2D else m.solve(tol, 30)
        assert out["converged"], out["reason"]
        sols.append((m.field(), out))
    diff = float(torch.linalg.vector_norm(sols[0][0] - sols[1][0]))
    print(f"cross-check {w}x{h}: CG {sols[0][1]['iterations']} iterations (residual {sols[0][1]['residual']:.3e}), "
          f"multigrid {sols[1][1]['cycles']} cycles (residual {sols[1][1]['residual']:.3e}), ||u_cg - u_mg||_2 {diff:.3e}, "
          f"bound {2 * tol / a:.3e}")
    assert diff <= 2 * tol / a


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_residual_is_multigrids(gpu, dtype):
    w, h = 127, 63
    gen = torch.Generator(device="cpu").manual_seed(9)
    field, src = _rand((h, w), gen, DT[dtype]), _rand((h, w), gen, DT[dtype], 0.01)
    res = []
    for cls, cfg in ((ConjugateGradient2D, CgConfig(width=w, height=h, dtype=dtype)),
                     (Multigrid2D, MultigridConfig(width=w, height=h, dtype=dtype))):
        m = cls(cfg, device="cuda")
        m.set_boundary(**BOUNDARY)
        m.set_field(field)
        m.set_source(src)
        res.append(m.residual())
    print(f"residual {dtype}: CG {res[0]}, multigrid {res[1]}")
    assert res[0]["l2"] > 0 and res[0] == res[1]


def test_fp32_converges_and_ends_at_its_floor(gpu):
    """9100 unknowns: in exact arithmetic CG ends within 9100 iterations, the cap
    here; fp32 took 183 in a CPU probe."""
    w, h = 130, 70
    m = _problem(w, h, "f32", "cuda")
    r0 = m.residual()["l2"]
    out = m.solve(1e-5 * r0, w * h)
    print(f"fp32 130x70: {out['iterations']} iterations, {out['restarts']} restarts, residual {out['residual']:.3e} "
          f"(tol {1e-5 * r0:.3e}), {out['reason']}")
    assert out["converged"] and out["residual"] <= 1e-5 * r0, out["reason"]
    end = m.solve(0.0, 600)
    print(f"fp32 130x70, tol 0: {end['reason']} after {end['iterations']} iterations, {end['restarts']} restarts, "
          f"residual {end['residual']:.3e}")
    assert end["reason"] in ("stalled", "max_iters reached") and not end["converged"]
    assert bool(torch.isfinite(m.full()).all())


# -------------------------------------------------------------- errors, CLI
def test_errors_on_the_device(gpu):
    from cuda_mpi_scratch_amd.parallel import DistContext

    with pytest.raises(ValueError, match="c_center \\+ 4 c_neighbor <= 1"):
        hip().CgSolver(128, 128, "f64", 0.3, 0.2)
    with pytest.raises(ValueError, match="c_neighbor > 0"):
        CgConfig(width=128, height=128, c_neighbor=0.0)
    with pytest.raises(ValueError, match="one process"):
        ConjugateGradient2D(CgConfig(width=128, height=64), DistContext(rank=0, world_size=2), device="cuda")
    m = ConjugateGradient2D(CgConfig(width=128, height=64), device="cuda")
    with pytest.raises(ValueError, match="shape"):
        m.set_source(torch.zeros(128, 64))
    with pytest.raises(ValueError, match="norm"):
        m.solve(1e-8, 5, norm="l1")
    with pytest.raises(ValueError, match="norm"):
        m.solver.solve(1e-8, 5, "l1", 4)
    with pytest.raises(ValueError, match="check_every"):
        m.solve(1e-8, 5, check_every=0)


def test_cli_solves_and_writes_its_json(gpu, tmp_path):
    path = tmp_path / "cg.json"
    cmd = [sys.executable, "-m", "cuda_mpi_scratch_amd.models.cg2d", "--size", "256x256", "--dtype", "f64",
           "--source", "1e-6", "--tol", "1e-8", "--c-center", "0.5", "--c-neighbor", "0.1", "--json", str(path)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    rec = json.loads(path.read_text().splitlines()[-1])
    assert rec == json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert rec["metric"] == "cg2d_solve_s" and rec["converged"] and rec["residual"] <= 1e-8
    assert 0 < rec["iterations"] <= 256 * 256 and rec["reason"].startswith("converged")
    assert rec["graph"] == "captured" and rec["config"]["width"] == 256 and rec["config"]["c_center"] == 0.5
    assert rec["device"].startswith("cuda")
