"""Multigrid-preconditioned CG on the GPU: each preconditioner kernel and each
pcg_* kernel bit for bit against its pure-torch reference (and what it may read
and write), the fused sums against the worst-case bound of a double summation,
the status protocol, the launchers' refusals, and the native solver: against a
dense direct solve, against the CPU twin's iteration counts, independent of the
host's check cadence and of the graph, a screened operator with a non-zero ring,
fp32, the errors and the CLI.

Everywhere: padding and whatever a kernel may not read holds NaN (the ring of a
reflecting side included: the ghost there is made from the core), outputs start
as a sentinel, and nothing outside the core may be written."""
import json
import math
import os
import subprocess
import sys

import pytest
import torch

from cuda_mpi_scratch_amd import core, hip, ops
from cuda_mpi_scratch_amd.models.pcg2d import MultigridPcg2D, PcgConfig
from tests.test_cg_cpu import direct_solution, ring_problem, setup
from tests.test_gpu_cg import SHAPES, _fields as _cg_fields, _same_bits, _sum_check
from tests.test_gpu_multigrid import (DT, SENTINEL, _assert_only_core_written, _core, _fields, _geom, _rand,
                                      _smooth_table, _tile)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CACHE = {}
FLAGS = [(False, False), (True, False), (False, True), (True, True)]  # (reflect_rows, reflect_cols)
NAN = float("nan")


def _poison_reflecting_ring(full, rr, rc):
    """A copy of `full` whose ring row H / column W is NaN on a reflecting side."""
    full = full.clone()
    if rr:
        full[-1, :] = NAN
    if rc:
        full[:, -1] = NAN
    return full


# ------------------------------------------------------------------ smoother
@pytest.mark.parametrize("rr,rc", FLAGS)
@pytest.mark.parametrize("nu", [1, 2, 3, 4])
@pytest.mark.parametrize("w,h", [(1, 1), (2, 2), (3, 3), (64, 32), (65, 33), (63, 31), (130, 70)])
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_smoother_with_flags_is_bitwise_the_reference(gpu, dtype, w, h, nu, rr, rc):
    """A workgroup stores a 64 x 32 tile and stages an NU-deep apron. (1, 1), (2,
    2), (3, 3): the reflecting ghost beside the first cells, the whole grid
    inside every apron. (64, 32): exactly one tile, the reflecting edge on the
    tile's last column and row and the ghost in its own apron. (65, 33): the
    last core column / row is the first cell of a new tile, so the ghost lives
    in that tile's window and, mirrored, in the apron of its neighbour, which
    must advance it to the same depth. (63, 31): the ghost is the last cell of
    the output window. (130, 70): 3 x 3 tiles, the reflecting edge 2 columns / 6
    rows into the last tile: inside the apron of the tile before it for NU >= 2
    (columns) and not at all for rows. Each with 1..4 fused sweeps of different
    weights and all four flag pairs; no flags is mg_smooth's case."""
    dt = DT[dtype]
    u, gsrc = _fields(w, h, dt)
    ce, nb, wt = _smooth_table(w, h, nu)
    key = ("smooth", w, h, dtype, nu, rr, rc)
    if key not in _CACHE:
        _CACHE[key] = ops.mgp_smooth_reference(u, gsrc, ce, nb, wt, rr, rc)[1:-1, 1:-1].clone()
    g = _geom(w, h, dt)
    u_in = _tile(gpu, g, dt, full=_poison_reflecting_ring(u, rr, rc))
    src = _tile(gpu, g, dt, core_vals=gsrc)
    out = _tile(gpu, g, dt, fill=SENTINEL)
    ops.mgp_smooth(u_in, out, src, g, ce, nb, wt, rr, rc)
    torch.cuda.synchronize()
    assert hip().last_pcg_dispatch() == "mgp_smooth"
    _assert_only_core_written(out, g, _CACHE[key], f"mgp_smooth {dtype} {w}x{h} NU={nu} flags {rr},{rc}")
    if not (rr or rc):
        assert torch.equal(_CACHE[key], ops.mg_smooth_reference(u, gsrc, ce, nb, wt)[1:-1, 1:-1])
    # The start from zero reads no iterate at all: the reference on a zero field, bit for bit (-0 included).
    zkey = ("smooth0", w, h, dtype, nu, rr, rc)
    if zkey not in _CACHE:
        _CACHE[zkey] = ops.mgp_smooth_reference(torch.zeros_like(u), gsrc, ce, nb, wt, rr, rc)[1:-1, 1:-1].clone()
    out0 = _tile(gpu, g, dt, fill=SENTINEL)
    ops.mgp_smooth(None, out0, src, g, ce, nb, wt, rr, rc)
    torch.cuda.synchronize()
    assert hip().last_pcg_dispatch() == "mgp_smooth_zero"
    _assert_only_core_written(out0, g, _CACHE[zkey], f"mgp_smooth from zero {dtype} {w}x{h} NU={nu} flags {rr},{rc}")
    assert _same_bits(_core(out0, g).cpu(), _CACHE[zkey]), "a zero's sign differs"


@pytest.mark.parametrize("w,h", [(64, 32), (130, 70), (259, 131)])
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_smoother_dot_epilogue(gpu, dtype, w, h):
    """sum src * out over the core: one, 3 x 3 and 5 x 5 workgroups with ragged
    last tiles (cells outside the core must not enter). The cells are the
    plain launch's; beta is the double quotient (0 while iteration == 0), and a
    status != 0 leaves the scalar block alone."""
    dt = DT[dtype]
    u, gsrc = _fields(w, h, dt)
    ce, nb, wt = _smooth_table(w, h, 2)
    want = ops.mgp_smooth_reference(u, gsrc, ce, nb, wt, True, True)[1:-1, 1:-1].clone()
    g = _geom(w, h, dt)
    u_in = _tile(gpu, g, dt, full=_poison_reflecting_ring(u, True, True))
    src = _tile(gpu, g, dt, core_vals=gsrc)
    ws = ops.PcgWorkspace(g, gpu)
    for iteration, rz_old, status in [(0, 2.0, 0), (3, 2.0, 0), (3, 2.0, 1), (3, 2.0, 3)]:
        out = _tile(gpu, g, dt, fill=SENTINEL)
        ws.write(rz=rz_old, beta=7.0, iteration=iteration, status=status, rr=1.5, max_iters=9)
        before = ws.read()
        ops.mgp_smooth(u_in, out, src, g, ce, nb, wt, True, True, ws)
        torch.cuda.synchronize()
        assert hip().last_pcg_dispatch() == "mgp_smooth_dot"
        _assert_only_core_written(out, g, want, f"mgp_smooth dot {dtype} {w}x{h}")
        sc = ws.read()
        assert int(ws.counter.item()) == 0, "the ticket was not put back"
        if status != 0:
            assert sc == before
            continue
        _sum_check(f"mgp_smooth rz {dtype} {w}x{h}", sc["rz"], gsrc.double() * want.double())
        assert sc["beta"] == (0.0 if iteration == 0 else sc["rz"] / rz_old)
        assert {k: v for k, v in sc.items() if k not in ("rz", "beta")} == \
            {k: v for k, v in before.items() if k not in ("rz", "beta")}


# ------------------------------------------------- restriction, prolongation
FINE = [(2, 2), (4, 6), (5, 4), (64, 32), (66, 34), (130, 70), (131, 70)]


@pytest.mark.parametrize("rr,rc", [(False, False), (True, True)])
@pytest.mark.parametrize("w,h", FINE)
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_clipped_restriction_is_bitwise_the_reference(gpu, dtype, w, h, rr, rc):
    """A workgroup owns 32 x 16 coarse cells and the 65 x 33 fine residuals they
    reach. (2, 2): one coarse cell whose far neighbours are all outside the
    core. (4, 6), (5, 4), (131, 70): both parities on each axis. (64, 32):
    exactly one coarse tile, its last cell on the last fine cell, the far
    residual column / row outside the core (0, not the ring's). (66, 34): one
    coarse cell into a second tile on each axis. (130, 70): 3 x 3 coarse tiles.
    The flags are the FINE level's: the residual of its last row / column reads
    the reflected ghost, never the ring there (NaN)."""
    dt = DT[dtype]
    u, gsrc = _fields(w, h, dt)
    c0, c1 = 0.15, 0.2
    key = ("restrict", w, h, dtype, rr, rc)
    if key not in _CACHE:
        _CACHE[key] = ops.mgp_residual_restrict_reference(u, gsrc, c0, c1, rr, rc)
    want = _CACHE[key]
    assert tuple(want.shape) == (h // 2, w // 2)
    g, gc = _geom(w, h, dt), _geom(w // 2, h // 2, dt)
    ut = _tile(gpu, g, dt, full=_poison_reflecting_ring(u, rr, rc))
    src = _tile(gpu, g, dt, core_vals=gsrc)
    out = _tile(gpu, gc, dt, fill=SENTINEL)
    ops.mgp_residual_restrict(ut, src, g, out, gc, c0, c1, rr, rc)
    torch.cuda.synchronize()
    assert hip().last_pcg_dispatch() == "mgp_residual_restrict"
    _assert_only_core_written(out, gc, want, f"mgp_residual_restrict {dtype} {w}x{h} flags {rr},{rc}")
    if w % 2 == 1 and h % 2 == 1 and not rr:
        assert torch.equal(want, ops.mg_residual_restrict_reference(u, gsrc, c0, c1))


@pytest.mark.parametrize("w,h", FINE)
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_prolongation_to_even_sides_is_bitwise_the_reference(gpu, dtype, w, h):
    """mg_prolong_add's kernel is zero outside the coarse core by index, so an even
    fine side needs nothing new: its last fine cell is a coarse point (odd
    index), the one before it the mean of two coarse cells. The same sizes as
    the restriction: both parities on each axis, one and several 64 x 4 blocks."""
    dt = DT[dtype]
    u, _ = _fields(w, h, dt)
    ch, cw = h // 2, w // 2
    e = _rand((ch, cw), torch.Generator(device="cpu").manual_seed(7 * w + h), dt)
    want = ops.mgp_prolong_add_reference(u[1:-1, 1:-1], e)
    g, gc = _geom(w, h, dt), _geom(cw, ch, dt)
    et = _tile(gpu, gc, dt, core_vals=e)  # ring and padding NaN: only the core of e is read
    ut = _tile(gpu, g, dt, core_vals=u[1:-1, 1:-1], fill=SENTINEL)
    ops.mgp_prolong_add(et, gc, ut, g)
    torch.cuda.synchronize()
    assert hip().last_pcg_dispatch() == "mgp_prolong_add"
    _assert_only_core_written(ut, g, want, f"mgp_prolong_add {dtype} {w}x{h}")


# -------------------------------------------------------------- coarse solve
@pytest.mark.parametrize("rr,rc", FLAGS)
@pytest.mark.parametrize("w,h", [(1, 1), (16, 16), (31, 1), (63, 63)])
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_coarse_solve_with_flags_is_bitwise_the_reference(gpu, dtype, w, h, rr, rc):
    """One workgroup, the grid in LDS: a single cell (all four neighbours ring or
    ghost), 16 x 16 (2048^2's coarsest), one row (the ghost row under every
    cell) and the largest grid the kernel holds (above the 64 KiB default of
    dynamic LDS in fp64). Two repeats of the level's own 32-sweep plan, so the
    ping-pong buffers both carry ghosts. With a workspace: the dot epilogue."""
    dt = DT[dtype]
    level = {"width": w, "height": h, "reflect_rows": rr, "reflect_cols": rc, "c_center": 0.2}
    plan = ops.pcg_coarse_plan(level, 0.2, 1e-3)
    gsrc = _fields(w, h, dt)[1]
    key = ("coarse", w, h, dtype, rr, rc)
    if key not in _CACHE:
        _CACHE[key] = ops.mgp_coarse_solve_reference(gsrc, plan["center"], plan["neighbor"], plan["weight"], 2, rr, rc)
    want = _CACHE[key]
    g = _geom(w, h, dt)
    src = _tile(gpu, g, dt, core_vals=gsrc)
    out = _tile(gpu, g, dt, fill=SENTINEL)
    ops.mgp_coarse_solve(src, out, g, plan["center"], plan["neighbor"], plan["weight"], 2, rr, rc)
    torch.cuda.synchronize()
    assert hip().last_pcg_dispatch() == "mgp_coarse_solve"
    _assert_only_core_written(out, g, want, f"mgp_coarse_solve {dtype} {w}x{h} flags {rr},{rc}")
    ws = ops.PcgWorkspace(g, gpu)
    ws.write(rz=0.5, iteration=2, status=0, max_iters=9)
    out2 = _tile(gpu, g, dt, fill=SENTINEL)
    ops.mgp_coarse_solve(src, out2, g, plan["center"], plan["neighbor"], plan["weight"], 2, rr, rc, ws)
    _assert_only_core_written(out2, g, want, f"mgp_coarse_solve dot {dtype} {w}x{h}")
    sc = ws.read()
    _sum_check(f"mgp_coarse_solve rz {dtype} {w}x{h}", sc["rz"], gsrc.double() * want.double())
    assert sc["beta"] == sc["rz"] / 0.5


# -------------------------------------------------------------- pcg_* kernels
@pytest.mark.parametrize("w,h", SHAPES)
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_pcg_start_is_bitwise_the_reference(gpu, dtype, w, h):
    """test_gpu_cg.SHAPES cover the row-band body's edges (see there); the body is
    cg_start's, so is the reference."""
    dt = DT[dtype]
    f = _cg_fields(w, h, dt)
    c0, c1 = 0.5, 0.1
    want, _, linf = ops.cg_start_reference(f["u"], f["g"], c0, c1)
    g = _geom(w, h, dt)
    u, src = _tile(gpu, g, dt, full=f["u"]), _tile(gpu, g, dt, core_vals=f["g"])
    r = _tile(gpu, g, dt, fill=SENTINEL)
    u0, src0 = u.clone(), src.clone()
    ws = ops.PcgWorkspace(g, gpu)
    ws.write(tol=0.0, max_iters=9, norm="l2", iteration=5, beta=3.0, rz=4.0, alpha=1.0, pq=2.0, status=2)
    ops.pcg_start(u, src, r, g, c0, c1, ws)
    torch.cuda.synchronize()
    assert hip().last_cg_dispatch() == "pcg_start"
    _assert_only_core_written(r, g, want, f"pcg_start r {dtype} {w}x{h}")
    assert _same_bits(u, u0) and _same_bits(src, src0), "pcg_start changed u or g"
    sc = ws.read()
    _sum_check(f"pcg_start rr {dtype} {w}x{h}", sc["rr"], want.double() ** 2)
    assert sc["linf"] == linf
    assert (sc["rz"], sc["pq"], sc["alpha"], sc["beta"], sc["iteration"], sc["status"], sc["max_iters"], sc["tol"]) == \
        (0.0, 0.0, 0.0, 0.0, 0, 0, 9, 0.0)
    assert int(ws.counter.item()) == 0, "the ticket was not put back"


@pytest.mark.parametrize("beta", [0.0, 0.37])
@pytest.mark.parametrize("w,h", SHAPES)
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_pcg_apply_is_bitwise_the_reference(gpu, dtype, w, h, beta):
    dt = DT[dtype]
    f = _cg_fields(w, h, dt)
    c0, c1 = 0.5, 0.1
    want_p, want_q, _ = ops.cg_apply_reference(f["r"], f["p"], beta, c0, c1)  # z in place of r
    g = _geom(w, h, dt)
    z, p_old = _tile(gpu, g, dt, core_vals=f["r"]), _tile(gpu, g, dt, core_vals=f["p"])
    p_new, q = _tile(gpu, g, dt, fill=SENTINEL), _tile(gpu, g, dt, fill=SENTINEL)
    z0, p0 = z.clone(), p_old.clone()
    ws = ops.PcgWorkspace(g, gpu)
    rz = 1.25
    ws.write(beta=beta, rz=rz, rr=77.0, tol=0.0, max_iters=100, iteration=3)
    ops.pcg_apply(z, p_old, p_new, q, g, c0, c1, ws)
    torch.cuda.synchronize()
    assert hip().last_cg_dispatch() == "pcg_apply"
    _assert_only_core_written(p_new, g, want_p, f"pcg_apply p_new {dtype} {w}x{h} beta={beta}")
    _assert_only_core_written(q, g, want_q, f"pcg_apply q {dtype} {w}x{h} beta={beta}")
    assert _same_bits(z, z0) and _same_bits(p_old, p0), "pcg_apply changed z or p_old"
    sc = ws.read()
    _sum_check(f"pcg_apply pq {dtype} {w}x{h}", sc["pq"], want_p.double() * want_q.double())
    assert sc["pq"] > 0 and sc["alpha"] == rz / sc["pq"], "alpha is not the double quotient of the stored rz and pq"
    assert (sc["status"], sc["iteration"], sc["rr"], sc["rz"], sc["beta"]) == (0, 3, 77.0, rz, beta)
    assert int(ws.counter.item()) == 0


@pytest.mark.parametrize("w,h", SHAPES)
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_pcg_update_is_bitwise_the_reference(gpu, dtype, w, h):
    dt = DT[dtype]
    f = _cg_fields(w, h, dt)
    alpha = 0.61
    want_u, want_r, _, linf = ops.cg_update_reference(f["u"][1:-1, 1:-1], f["r"], f["p"], f["q"], alpha)
    g = _geom(w, h, dt)
    u = _tile(gpu, g, dt, core_vals=f["u"][1:-1, 1:-1], fill=SENTINEL)
    r = _tile(gpu, g, dt, core_vals=f["r"], fill=SENTINEL)
    p, q = _tile(gpu, g, dt, core_vals=f["p"]), _tile(gpu, g, dt, core_vals=f["q"])
    p0, q0 = p.clone(), q.clone()
    ws = ops.PcgWorkspace(g, gpu)
    ws.write(alpha=alpha, rr=2.5, rz=1.5, beta=0.25, tol=0.0, max_iters=100, iteration=4, norm="linf")
    ops.pcg_update(u, r, p, q, g, ws)
    torch.cuda.synchronize()
    assert hip().last_cg_dispatch() == "pcg_update"
    _assert_only_core_written(u, g, want_u, f"pcg_update u {dtype} {w}x{h}")
    _assert_only_core_written(r, g, want_r, f"pcg_update r {dtype} {w}x{h}")
    assert _same_bits(p, p0) and _same_bits(q, q0), "pcg_update changed p or q"
    sc = ws.read()
    _sum_check(f"pcg_update rr {dtype} {w}x{h}", sc["rr"], want_r.double() ** 2)
    assert sc["linf"] == linf
    assert (sc["beta"], sc["rz"]) == (0.25, 1.5), "pcg_update must leave beta and rz to the dot epilogue"
    assert (sc["iteration"], sc["status"], sc["alpha"]) == (5, 0, alpha)
    assert int(ws.counter.item()) == 0


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_status_protocol(gpu, dtype):
    dt = DT[dtype]
    w, h = 130, 70
    f = _cg_fields(w, h, dt)
    g = _geom(w, h, dt)
    c0, c1 = 0.2, 0.2
    ws = ops.PcgWorkspace(g, gpu)
    u, src = _tile(gpu, g, dt, full=f["u"]), _tile(gpu, g, dt, core_vals=f["g"])
    r, z = _tile(gpu, g, dt, fill=SENTINEL), _tile(gpu, g, dt, core_vals=f["r"])
    p = _tile(gpu, g, dt, core_vals=f["p"])
    p2, q = _tile(gpu, g, dt, fill=SENTINEL), _tile(gpu, g, dt, fill=SENTINEL)
    _, rr, linf = ops.cg_start_reference(f["u"], f["g"], c0, c1)
    for norm, tol, want in [("l2", 2 * math.sqrt(rr), 1), ("l2", 0.5 * math.sqrt(rr), 0), ("linf", 2 * linf, 1),
                            ("linf", 0.5 * linf, 0)]:
        ws.write(tol=tol, max_iters=10, norm=norm, status=0)
        ops.pcg_start(u, src, r, g, c0, c1, ws)
        assert ws.read()["status"] == want, (norm, tol)
    ws.write(tol=0.0, max_iters=0, norm="l2")
    ops.pcg_start(u, src, r, g, c0, c1, ws)
    assert ws.read()["status"] == 2
    for tol, max_iters, want in [(0.0, 1, 2), (1e30, 1, 1), (1e30, 5, 1), (0.0, 5, 0)]:
        ws.write(tol=tol, max_iters=max_iters, norm="l2")
        ops.pcg_start(u, src, r, g, c0, c1, ws)
        ws.write(status=0, rz=1.0)
        ops.pcg_apply(z, p, p2, q, g, c0, c1, ws)
        ops.pcg_update(u.clone(), r.clone(), p2, q, g, ws)
        sc = ws.read()
        assert (sc["status"], sc["iteration"]) == (want, 1), (tol, max_iters, sc)
    # with a status != 0 at entry the kernels leave every tile and the scalar block bitwise unchanged
    ce, nb, wt = _smooth_table(w, h, 2)
    tiles = [u, r, p, p2, q]
    for status in (1, 2, 3):
        ws.write(status=status, alpha=0.5, beta=0.25, rz=2.0)
        before, sc0 = [t.clone() for t in tiles], ws.read()
        ops.mgp_smooth(u, _tile(gpu, g, dt, fill=SENTINEL), z, g, ce, nb, wt, False, False, ws)
        ops.pcg_apply(z, p, p2, q, g, c0, c1, ws)
        ops.pcg_update(u, r, p2, q, g, ws)
        torch.cuda.synchronize()
        assert all(_same_bits(a, b) for a, b in zip(tiles, before)), f"status {status}: a tile changed"
        assert ws.read() == sc0 and int(ws.counter.item()) == 0
    # p' = 0: pq = 0 is a breakdown, alpha = 0, and nothing is NaN
    zero = torch.zeros(h, w, dtype=dt)
    zz, zp = _tile(gpu, g, dt, core_vals=zero), _tile(gpu, g, dt, core_vals=zero)
    ws.write(status=0, beta=0.37, rz=1.0, alpha=9.0, max_iters=10)
    ops.pcg_apply(zz, zp, p2, q, g, c0, c1, ws)
    sc = ws.read()
    assert (sc["status"], sc["alpha"], sc["pq"]) == (3, 0.0, 0.0)
    assert bool((_core(p2, g) == 0).all()) and bool((_core(q, g) == 0).all())


def test_launchers_refuse_bad_arguments(gpu):
    dt = torch.float64
    w, h = 64, 32
    g, gc = _geom(w, h, dt), _geom(32, 16, dt)
    a, b, c, d = (_tile(gpu, g, dt, fill=0.0) for _ in range(4))
    e = _tile(gpu, gc, dt, fill=0.0)
    ws = ops.PcgWorkspace(g, gpu)
    bare = core().TileGeom.aligned(w, h, 0, 0, 8)
    with pytest.raises(Exception, match="no ghost ring"):
        ops.pcg_start(a, b, c, bare, 0.2, 0.2, ws)
    with pytest.raises(Exception, match="no ghost ring"):
        ops.pcg_apply(a, b, c, d, bare, 0.2, 0.2, ws)
    with pytest.raises(Exception, match="no ghost ring"):
        ops.pcg_update(a, b, c, d, bare, ws)
    with pytest.raises(Exception, match="no ghost ring"):
        ops.mgp_smooth(a, b, c, bare, [0.2], [0.2], [1.0])
    with pytest.raises(Exception, match="three tiles"):
        ops.pcg_start(a, b, a, g, 0.2, 0.2, ws)
    with pytest.raises(Exception, match="p_old != p_new"):
        ops.pcg_apply(a, b, b, d, g, 0.2, 0.2, ws)
    with pytest.raises(Exception, match="four tiles"):
        ops.pcg_update(a, a, c, d, g, ws)
    with pytest.raises(Exception, match="u_in != u_out"):
        ops.mgp_smooth(a, a, c, g, [0.2], [0.2], [1.0])
    with pytest.raises(Exception, match="sweeps per launch"):
        ops.mgp_smooth(a, b, c, g, [0.2] * 5, [0.2] * 5, [1.0] * 5)
    wrong = _geom(31, 16, dt)
    with pytest.raises(Exception, match=r"\(width / 2\) x \(height / 2\)"):
        ops.mgp_residual_restrict(a, b, g, e, wrong)
    with pytest.raises(Exception, match=r"\(width / 2\) x \(height / 2\)"):
        ops.mgp_prolong_add(e, wrong, a, g)
    with pytest.raises(Exception, match="at most 63"):
        ops.mgp_coarse_solve(a, b, g, [0.2], [0.2], [1.0], 1)
    host = torch.zeros(g.alloc_elems(), dtype=dt)
    with pytest.raises(TypeError, match="GPU tensors only"):
        ops.pcg_start(host, b, c, g, 0.2, 0.2, ws)
    with pytest.raises(TypeError, match="GPU tensors only"):
        ops.mgp_smooth(a, host, c, g, [0.2], [0.2], [1.0])


# --------------------------------------------------------------------- solver
@pytest.mark.parametrize("c0,c1", [(0.2, 0.2), (0.5, 0.1)])
def test_solver_against_the_dense_direct_solve(gpu, c0, c1):
    """40 x 24, a non-zero ring and source, the pure and a screened operator:
    ||u - u_direct||_2 <= tol / a (test_cg_cpu's theorem)."""
    w, h, tol = 40, 24, 1e-10
    prob = ring_problem(w, h)
    m = MultigridPcg2D(PcgConfig(width=w, height=h, dtype="f64", c_center=c0, c_neighbor=c1), device="cuda")
    assert m.solver is not None
    setup(m, prob)
    out = m.solve(tol, 200)
    a = ops.relaxation_spectrum(w, h, c0, c1)[0]
    err = float(torch.linalg.vector_norm(m.field().cpu() - direct_solution(w, h, c0, c1, prob)))
    print(f"device {w}x{h} ({c0}, {c1}): {out['iterations']} iterations, {out['restarts']} restarts, true l2 residual "
          f"{out['residual']:.3e}, ||u - u_direct||_2 {err:.3e}, bound {tol / a:.3e}; {m.note()}")
    assert out["converged"] and out["residual"] <= tol, out["reason"]
    assert err <= (tol / a) * (1 + 1e-6)
    assert out["iterations"] <= 20


@pytest.mark.parametrize("w,h", [(256, 256), (250, 250), (100, 37)])
def test_iteration_count_is_the_cpu_twins(gpu, w, h):
    """f = 1, zero ring, fp64, l2 <= 1e-8: every cell is the twin's bit for bit
    given the same scalars, and the sums differ in term order only, so the
    counts agree within 1."""
    twin = ops.pcg_reference(torch.zeros(h + 2, w + 2, dtype=torch.float64), torch.ones(h, w, dtype=torch.float64),
                             tol=1e-8, max_iters=100)
    m = MultigridPcg2D(PcgConfig(width=w, height=h, dtype="f64"), device="cuda")
    m.set_source(1.0)
    out = m.solve(1e-8, 100)
    diff = float((m.full().cpu() - twin["full"]).abs().max())
    print(f"{w}x{h}: device {out['iterations']} iterations (residual {out['residual']:.3e}), twin {twin['iterations']} "
          f"(residual {twin['residual']:.3e}); max |u_gpu - u_twin| {diff:.3e} of {float(twin['full'].abs().max()):.3e}")
    assert twin["converged"] and out["converged"], (twin["reason"], out["reason"])
    assert abs(out["iterations"] - twin["iterations"]) <= 1
    assert m.levels == ops.pcg_plan_levels(w, h) and len(m.solver.levels()) == len(m.levels)


def _ring_model(w, h, dtype, c0, c1, **kw):
    m = MultigridPcg2D(PcgConfig(width=w, height=h, dtype=dtype, c_center=c0, c_neighbor=c1, **kw), device="cuda")
    gen = torch.Generator(device="cpu").manual_seed(w + 3 * h)
    m.set_boundary(top=1.0, bottom=_rand((w,), gen, torch.float64), left=torch.linspace(1.0, 0.0, h, dtype=torch.float64),
                   right=-0.5)
    m.set_field(_rand((h, w), gen, torch.float64))
    src = _rand((h, w), gen, torch.float64, 1e-3)
    m.set_source(src)
    return m, src


def test_the_check_cadence_and_the_graph_change_no_bit(gpu):
    """250 x 130 (even x even, five levels) with a non-zero ring."""
    w, h, tol = 250, 130, 1e-9
    first = None
    for graph in (True, False):
        for every in (2, 4, 8):
            m, _ = _ring_model(w, h, "f64", 0.2, 0.2, graph=graph, check_every=every)
            out = m.solve(tol, 200)
            got = m.full()
            print(f"check_every {every}, graph {graph} ({m.graph_status()}): {out['iterations']} iterations, "
                  f"{len(out['history'])} checks, residual {out['residual']:.3e}")
            assert out["converged"], out["reason"]
            assert m.graph_status() == ("captured" if graph else "off")
            if first is None:
                first = (got, out["iterations"], out["residual"], out["restarts"])
            assert _same_bits(got, first[0]), "the field depends on the cadence or on the graph"
            assert (out["iterations"], out["residual"], out["restarts"]) == first[1:]
    assert first[1] <= 25


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_a_second_solve_depends_on_the_field_alone(gpu, dtype):
    """Nothing of one solve may leak into the next: after a converged solve, two
    more iterations give the same bits whether or not the host read the field
    (and ran other device work) in between, under a graph and eagerly."""
    w, h = 256, 256
    got = []
    for graph in (True, False):
        for read_between in (False, True):
            m, _ = _ring_model(w, h, dtype, 0.2, 0.2, graph=graph)
            m.solve(1e-5 * m.residual()["l2"], 200)
            if read_between:
                assert bool(torch.isfinite(m.full()).all())
            out = m.solve(0.0, 2)
            sc = m.scalars()
            print(f"{dtype} graph {graph}, read between {read_between}: rz {sc['rz']!r}, pq {sc['pq']!r}")
            assert out["iterations"] == 2 and out["reason"] == "max_iters reached"
            got.append((m.full(), sc))
    for f, sc in got[1:]:
        assert _same_bits(f, got[0][0]) and sc == got[0][1]


def test_screened_operator_with_a_ring(gpu):
    """(0.5, 0.1) on 250 x 130 with non-zero boundaries: the reported residual is
    the recomputed one, and the exact iteration cap holds."""
    w, h, c0, c1, tol = 250, 130, 0.5, 0.1, 1e-10
    m, src = _ring_model(w, h, "f64", c0, c1)
    out = m.solve(tol, 100)
    _, l2 = ops.residual5_reference(m.full().cpu(), 1, c0, c1, source=src)
    print(f"{w}x{h} ({c0}, {c1}): {out['iterations']} iterations, residual {out['residual']:.3e}, recomputed {l2:.3e}")
    assert out["converged"], out["reason"]
    assert l2 <= tol and out["residual"] == pytest.approx(l2, rel=1e-9)
    m2, _ = _ring_model(w, h, "f64", c0, c1)
    capped = m2.solve(0.0, 3)
    sc = m2.scalars()
    assert capped["iterations"] == 3 and capped["reason"] == "max_iters reached"
    assert (sc["iteration"], sc["status"], sc["max_iters"]) == (3, 2, 3) and sc["rz"] > 0


def test_fp32_ends_converged_or_stalled_with_a_finite_field(gpu):
    m, _ = _ring_model(256, 256, "f32", 0.2, 0.2)
    r0 = m.residual()["l2"]
    out = m.solve(1e-5 * r0, 200)
    print(f"fp32 256x256: {out['iterations']} iterations, {out['restarts']} restarts, residual {out['residual']:.3e} "
          f"(tol {1e-5 * r0:.3e}), {out['reason']}")
    assert out["reason"].startswith("converged") or out["reason"] == "stalled"
    assert bool(torch.isfinite(m.full()).all())
    end = m.solve(0.0, 60)
    print(f"fp32 256x256, tol 0: {end['reason']} after {end['iterations']} iterations, residual {end['residual']:.3e}, "
          f"scalars {m.scalars()}")
    assert end["reason"] in ("stalled", "max_iters reached") and not end["converged"]
    assert bool(torch.isfinite(m.full()).all())


# -------------------------------------------------------------- errors, CLI
def test_errors_on_the_device(gpu):
    from cuda_mpi_scratch_amd.parallel import DistContext

    with pytest.raises(ValueError, match="c_center \\+ 4 c_neighbor <= 1"):
        hip().PcgSolver(128, 128, "f64", 0.3, 0.2)
    with pytest.raises(ValueError, match="ConjugateGradient2D"):
        hip().PcgSolver(3000, 4, "f64")
    with pytest.raises(ValueError, match="nu_pre must equal nu_post"):
        PcgConfig(width=128, height=128, nu_pre=1, nu_post=2)
    with pytest.raises(ValueError, match="one process"):
        MultigridPcg2D(PcgConfig(width=128, height=64), DistContext(rank=0, world_size=2), device="cuda")
    m = MultigridPcg2D(PcgConfig(width=128, height=64), device="cuda")
    with pytest.raises(ValueError, match="shape"):
        m.set_source(torch.zeros(128, 64))
    with pytest.raises(ValueError, match="norm"):
        m.solve(1e-8, 5, norm="l1")
    with pytest.raises(ValueError, match="norm"):
        m.solver.solve(1e-8, 5, "l1", 4)
    with pytest.raises(ValueError, match="check_every"):
        m.solve(1e-8, 5, check_every=0)


def test_cli_solves_and_writes_its_json(gpu, tmp_path):
    path = tmp_path / "pcg.json"
    cmd = [sys.executable, "-m", "cuda_mpi_scratch_amd.models.pcg2d", "--size", "256x256", "--dtype", "f64",
           "--source", "1e-6", "--tol", "1e-8", "--json", str(path)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    rec = json.loads(path.read_text().splitlines()[-1])
    assert rec == json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert rec["metric"] == "pcg2d_solve_s" and rec["converged"] and rec["residual"] <= 1e-8
    assert 0 < rec["iterations"] <= 40 and rec["reason"].startswith("converged")
    assert rec["graph"] == "captured" and rec["config"]["width"] == 256 and rec["levels"][-1] == [16, 16]
    assert rec["device"].startswith("cuda")
