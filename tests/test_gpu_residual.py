"""Convergence control on the GPU: the fused residual-norm kernel
(ops.stencil5_residual) against the float64 CPU reference, what it may read,
NaN propagation and determinism; StencilSolver.residual() on every one-rank
schedule; run_until()'s stopping rule against a float64 reference history, on
one rank and on 2 x 2 ranks sharing the GPU; the CLI and the MPI app.

Tolerances come from the project's own TOL (2e-6 fp32, 1e-14 fp64, fields in
[0, 1)): each r is one stencil value minus an exact input, so |linf - ref| <=
2 TOL and, by the triangle inequality in the 2-norm, |l2 - ref| <= 2 TOL
sqrt(w h); both scaled by max|u| of the case."""
import json
import math
import os
import re
import shutil
import subprocess
import sys

import pytest
import torch

from cuda_mpi_scratch_amd import core, hip, ops
from cuda_mpi_scratch_amd.models.stencil2d import Stencil2D, StencilConfig
from tests.residual_worker import boundary, launch, padded, reference_history

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = torch.float32, torch.float64
TOL = {F32: 2e-6, F64: 1e-14}
NAME = {F32: "f32", F64: "f64"}

KERNEL_CASES = [
    (264, 200, 12, F32),
    (262, 200, 12, F32),   # ragged width
    (1030, 70, 4, F32),    # several column strips, ragged
    (40, 24, 12, F32),     # smaller than a strip
    (5, 3, 1, F32),        # tiny, minimal ring
    (256, 1, 1, F32),      # one row
    (200, 136, 16, F64),
    (202, 136, 7, F64),    # ragged
    (3, 5, 1, F64),
]
COEFFS = [(0.2, 0.2), (0.5, 0.125)]


def _geom(w, h, ring, dtype):
    return core().TileGeom.aligned(w, h, ring, ring, torch.tensor([], dtype=dtype).element_size())


def _full(buf, g):
    return buf.view(g.total_height(), g.pitch)[:, g.x_origin:g.x_origin + g.total_width()]


def _random_tile(gpu, w, h, ring, dtype, seed):
    """Core and ghost ring random in [0, 1), the alignment padding zero."""
    g = _geom(w, h, ring, dtype)
    gen = torch.Generator(device="cpu").manual_seed(seed)
    full = torch.rand(g.total_height(), g.total_width(), generator=gen, dtype=torch.float64).to(dtype)
    src = torch.zeros(g.alloc_elems(), dtype=dtype, device=gpu)
    _full(src, g).copy_(full)
    return g, full, src


def _bits(x):
    return torch.tensor(x, dtype=torch.float64).view(torch.int64).item()


@pytest.mark.parametrize("c0,c1", COEFFS)
@pytest.mark.parametrize("w,h,ring,dtype", KERNEL_CASES)
def test_kernel_matches_reference(gpu, w, h, ring, dtype, c0, c1):
    g, full, src = _random_tile(gpu, w, h, ring, dtype, 7 * w + h + ring)
    linf, sumsq = ops.stencil5_residual(src, g, c0, c1)
    rl, r2 = ops.residual5_reference(full, ring, c0, c1)
    l2 = math.sqrt(sumsq)
    print(f"residual {w}x{h} ring {ring} {NAME[dtype]} c=({c0}, {c1}): linf {linf:.9g} (ref {rl:.9g}, "
          f"diff {abs(linf - rl):.3e}), l2 {l2:.9g} (ref {r2:.9g}, diff {abs(l2 - r2):.3e})")
    assert abs(linf - rl) <= 2 * TOL[dtype]
    assert abs(l2 - r2) <= 2 * TOL[dtype] * math.sqrt(w * h)


@pytest.mark.parametrize("w,h,ring,dtype", KERNEL_CASES)
def test_kernel_reads_nothing_it_must_not(gpu, w, h, ring, dtype):
    """NaN in every ring cell not beside the core (layers >= 2, the four
    corners) and in the alignment padding: finite, and bitwise the result with
    zeros there."""
    g, full, src = _random_tile(gpu, w, h, ring, dtype, 3 * w + h)
    keep = torch.zeros(g.total_height(), g.total_width(), dtype=torch.bool)
    keep[ring:ring + h, ring - 1:ring + w + 1] = True   # the core and columns -1, w over core rows
    keep[ring - 1:ring + h + 1, ring:ring + w] = True   # rows -1, h over core columns
    results = []
    for poison in (0.0, float("nan")):
        buf = torch.full((g.alloc_elems(),), poison, dtype=dtype, device=gpu)
        _full(buf, g).copy_(torch.where(keep, full, torch.full_like(full, poison)))
        results.append(ops.stencil5_residual(buf, g, 0.2, 0.2))
    (l0, s0), (l1, s1) = results
    assert math.isfinite(l1) and math.isfinite(s1)
    assert (_bits(l0), _bits(s0)) == (_bits(l1), _bits(s1))
    rl, _ = ops.residual5_reference(full, ring, 0.2, 0.2)
    assert abs(l0 - rl) <= 2 * TOL[dtype]


@pytest.mark.parametrize("w,h,ring,dtype", [KERNEL_CASES[1], KERNEL_CASES[2], KERNEL_CASES[7]])
def test_kernel_non_finite_propagates(gpu, w, h, ring, dtype):
    g, _, src = _random_tile(gpu, w, h, ring, dtype, 11)
    view = _full(src, g)
    for x, y in ((w - 1, h - 1), (0, 0), (w // 2, h // 2)):
        saved = view[ring + y, ring + x].item()
        view[ring + y, ring + x] = float("nan")
        linf, sumsq = ops.stencil5_residual(src, g)
        assert math.isnan(linf), (x, y, linf)
        view[ring + y, ring + x] = float("inf")
        linf, _ = ops.stencil5_residual(src, g)
        assert not math.isfinite(linf), (x, y, linf)
        view[ring + y, ring + x] = saved
    assert math.isfinite(ops.stencil5_residual(src, g)[0])


@pytest.mark.parametrize("w,h,ring,dtype", [KERNEL_CASES[2], KERNEL_CASES[6]])
def test_kernel_deterministic(gpu, w, h, ring, dtype):
    g, _, src = _random_tile(gpu, w, h, ring, dtype, 19)
    first = tuple(map(_bits, ops.stencil5_residual(src, g)))
    assert tuple(map(_bits, ops.stencil5_residual(src, g))) == first
    torch.cuda.synchronize()
    for _ in range(2):
        s = torch.cuda.Stream()
        assert tuple(map(_bits, ops.stencil5_residual(src, g, stream=s))) == first


@pytest.mark.parametrize("dtype,c0,c1,value", [(F32, 0.2, 0.2, 1.0), (F64, 0.2, 0.2, 1.0), (F32, 0.5, 0.125, 0.7),
                                               (F64, 0.5, 0.125, 0.7)])
def test_kernel_fixed_point_is_exactly_zero(gpu, dtype, c0, c1, value):
    g = _geom(262, 70, 3, dtype)
    src = torch.full((g.alloc_elems(),), value, dtype=dtype, device=gpu)
    assert ops.stencil5_residual(src, g, c0, c1) == (0.0, 0.0)


def test_kernel_rejects_a_tile_without_ring(gpu):
    g = _geom(64, 48, 0, F32)
    src = torch.zeros(g.alloc_elems(), dtype=F32, device=gpu)
    with pytest.raises(ValueError, match="no ghost ring"):
        ops.stencil5_residual(src, g)
    with pytest.raises(Exception, match="no ghost ring"):
        hip().stencil5_residual(src.data_ptr(), g, 0.2, 0.2, "f32", torch.cuda.current_stream().cuda_stream)


# ------------------------------------------------------------------ solver
W, H = 48, 32

SOLVER_CONFIGS = {
    "periodic-fused-f32": dict(dtype="f32"),
    "periodic-fused-f64": dict(dtype="f64"),
    "periodic-unfused": dict(dtype="f32", fuse_periodic=False),
    "rehearse-peers": dict(dtype="f32", loopback=True, rehearse_peers=True),
    "fixed-S1": dict(dtype="f32", periodic=False),
    "fixed-blocked": dict(dtype="f32", periodic=False, block_fixed_edges=True),
}


def _make(w=W, h=H, seed=3, **kw):
    cfg = StencilConfig(global_width=w, global_height=h, dims="1x1", seed=seed, **kw)
    st = Stencil2D(cfg)
    if not cfg.periodic:
        st.set_boundary(**boundary(w, h))
    return st


def _expect(st):
    """(linf, l2) of the reference on the gathered field with the ring the
    topology gives it, and the case's max|u|."""
    bnd = None if st.cfg.periodic else boundary(st.cfg.global_width, st.cfg.global_height)
    p = padded(st.gather_global(), bnd)
    c0 = float(torch.tensor(st.cfg.c_center, dtype=st.dtype))
    c1 = float(torch.tensor(st.cfg.c_neighbor, dtype=st.dtype))
    return ops.residual5_reference(p.to(st.dtype), 1, c0, c1), max(1.0, p.abs().max().item())


@pytest.mark.parametrize("name", list(SOLVER_CONFIGS))
def test_solver_residual_equals_reference(gpu, name):
    st = _make(**SOLVER_CONFIGS[name])
    if name == "periodic-unfused":
        assert not st.solver.fused_periodic()
    if name.startswith("periodic-fused"):
        assert st.solver.fused_periodic()
    if name == "rehearse-peers":
        assert st.solver.multi_rank()
    if name == "fixed-blocked":
        assert st.time_block > 1 and st.fixed_edge_note()
    for iters in (0, 7, 24):
        st.run(iters)
        got = st.residual()
        (rl, r2), scale = _expect(st)
        print(f"{name} after run({iters}): linf {got['linf']:.9g} (ref {rl:.9g}), l2 {got['l2']:.9g} (ref {r2:.9g})")
        assert got["cells"] == W * H
        assert abs(got["linf"] - rl) <= 2 * TOL[st.dtype] * scale
        assert abs(got["l2"] - r2) <= 2 * TOL[st.dtype] * scale * math.sqrt(W * H)


@pytest.mark.parametrize("name", ["periodic-fused-f32", "rehearse-peers", "fixed-blocked"])
def test_solver_residual_leaves_the_field_alone(gpu, name):
    kw = dict(SOLVER_CONFIGS[name], sum_form=False)
    a, b = _make(**kw), _make(**kw)
    a.run(5), b.run(5)
    before = a.gather_global().clone()
    r1, r2 = a.residual(), a.residual()
    assert r1 == r2
    assert torch.equal(a.gather_global(), before)
    a.run(12), b.run(12)
    assert torch.equal(a.gather_global(), b.gather_global())


_HIST = {}


def _history(w, h, every, checks, periodic, dtype="f32"):
    """The float64 CPU reference history from the solver's own initial field."""
    key = (w, h, every, checks, periodic, dtype)
    if key not in _HIST:
        st = _make(w, h, dtype=dtype, periodic=periodic)
        _HIST[key] = reference_history(st.gather_global(), every, checks, None if periodic else boundary(w, h))
    return _HIST[key]


def _tol_between(hist, lo):
    tol = math.sqrt(hist[lo] * hist[lo + 1])
    print(f"reference at checks {lo} / {lo + 1}: {hist[lo]:.6g} / {hist[lo + 1]:.6g}, tol {tol:.6g}")
    assert hist[lo] / tol >= 1.05 and tol / hist[lo + 1] >= 1.05  # the reference's own margin
    return tol


@pytest.mark.parametrize("sum_form", [True, False])
def test_run_until_stopping_rule_fixed_edges(gpu, sum_form):
    hist = [x[0] for x in _history(W, H, 60, 18, False)]
    tol = _tol_between(hist, 16)
    st = _make(periodic=False, block_fixed_edges=True, sum_form=sum_form)
    out = st.run_until(tol, 5000, 60)
    print(f"run_until: {out['iterations']} iterations, {out['checks']} checks, residual {out['residual']:.6g} "
          f"(reference {hist[17]:.6g})")
    assert out["converged"] and out["iterations"] == 1020 and out["checks"] == 18, out
    assert st.iteration == 1020
    assert abs(out["residual"] - hist[17]) <= 2 * TOL[F32] * 100
    assert [it for it, _, _ in out["history"]] == list(range(0, 1021, 60))
    if not sum_form:
        other = _make(periodic=False, block_fixed_edges=True, sum_form=False)
        for _ in range(17):
            other.run(60)
        assert torch.equal(st.gather_global(), other.gather_global())


def test_run_until_stopping_rule_periodic(gpu):
    w, h = 64, 48
    hist = [x[0] for x in _history(w, h, 48, 7, True)]
    tol = _tol_between(hist, 5)
    st = _make(w, h)
    assert st.solver.fused_periodic()
    out = st.run_until(tol, 5000, 48)
    assert out["converged"] and out["iterations"] == 288 and out["checks"] == 7, out
    assert abs(out["residual"] - hist[6]) <= 2 * TOL[F32]


def test_run_until_l2_norm(gpu):
    l2 = [x[1] for x in _history(W, H, 60, 18, False)]
    tol = _tol_between(l2, 16)
    st = _make(periodic=False, block_fixed_edges=True)
    out = st.run_until(tol, 5000, 60, norm="l2")
    assert out["converged"] and out["iterations"] == 1020 and out["checks"] == 18 and out["norm"] == "l2", out
    assert abs(out["residual"] - l2[17]) <= 2 * TOL[F32] * 100 * math.sqrt(W * H)


def test_run_until_cap_converged_and_non_finite(gpu):
    st = _make(periodic=False, block_fixed_edges=True)
    out = st.run_until(0.0, 120, 60)
    assert not out["converged"] and out["iterations"] == 120 and out["checks"] == 3, out
    assert "max_iters" in out["reason"]
    st = Stencil2D(StencilConfig(global_width=W, global_height=H, dims="1x1", periodic=False, block_fixed_edges=True))
    st.core_view().fill_(1.0)
    st.set_boundary(top=1.0, bottom=1.0, left=1.0, right=1.0)
    out = st.run_until(1e-9, 600, 60)
    assert out["converged"] and out["iterations"] == 0 and out["checks"] == 1 and out["residual"] == 0.0, out
    st = _make(periodic=False, block_fixed_edges=True)
    st.core_view()[5, 7] = float("nan")
    out = st.run_until(1e-3, 600, 60)
    assert not out["converged"] and out["iterations"] == 0 and "non-finite" in out["reason"], out


def test_run_until_default_chunk_is_sixteen_time_blocks(gpu):
    st = _make()
    tb = st.time_block
    assert hip().DEFAULT_CHECK_BLOCKS == Stencil2D.DEFAULT_CHECK_BLOCKS == 16
    out = st.run_until(0.0, 40 * tb)
    assert [it for it, _, _ in out["history"]] == [0, 16 * tb, 32 * tb, 40 * tb]


def test_bad_arguments_raise(gpu):
    st = _make()
    with pytest.raises(ValueError, match="tol"):
        st.run_until(-1.0, 10)
    with pytest.raises(ValueError, match="max_iters"):
        st.run_until(1.0, -1)
    with pytest.raises(Exception, match="tol must be >= 0"):
        st.solver.run_until(-1.0, 10)
    with pytest.raises(Exception, match="max_iters must be >= 0"):
        st.solver.run_until(1.0, -1)
    box = Stencil2D(StencilConfig(global_width=W, global_height=H, dims="1x1", kind="box", box_weights=[1 / 9] * 9))
    with pytest.raises(ValueError, match="box"):
        box.run_until(1.0, 10)
    with pytest.raises(Exception, match="box"):
        box.solver.residual()
    with pytest.raises(Exception, match="box"):
        box.solver.run_until(1.0, 10)


# -------------------------------------------------------------- multi-rank
_ONE_RANK = {}


def _one_rank(tol):
    if tol not in _ONE_RANK:
        _ONE_RANK[tol] = launch(1, {"w": W, "h": H, "dims": "1x1", "backend": "local", "seed": 3, "tol": tol,
                                    "max_iters": 5000, "check_every": 60})[0]
    return _ONE_RANK[tol]


@pytest.mark.parametrize("direct", [None, False])
def test_multi_rank_run_until_equals_one_rank(gpu, direct):
    """2 x 2 ranks share the GPU (IPC backend, tiles 24 x 16), per-step form:
    every rank stops at the one-rank iteration with the one-rank linf."""
    hist = [x[0] for x in _history(W, H, 60, 18, False)]
    tol = _tol_between(hist, 16)
    one = _one_rank(tol)
    assert one["until"]["converged"] and one["until"]["iterations"] == 1020 and one["until"]["checks"] == 18
    res = launch(4, {"w": W, "h": H, "dims": "2x2", "backend": "ipc", "seed": 3, "tol": tol, "max_iters": 5000,
                     "check_every": 60, "direct_halo": direct})
    for r in res:
        assert r["direct"] == (direct is None), r
        assert r["until"] == res[0]["until"] and r["first"] == res[0]["first"], r
        assert r["iteration"] == 1020
    got = res[0]
    assert got["until"]["iterations"] == 1020 and got["until"]["checks"] == 18 and got["until"]["converged"]
    assert _bits(got["until"]["residual"]) == _bits(one["until"]["residual"])
    assert _bits(got["first"]["linf"]) == _bits(one["first"]["linf"])
    assert got["first"]["cells"] == W * H
    for (ia, la, sa), (ib, lb, sb) in zip(got["until"]["history"], one["until"]["history"]):
        assert ia == ib and _bits(la) == _bits(lb)
        assert abs(sa - sb) <= 1e-12 * sb
    assert got["grid"] == one["grid"]


# --------------------------------------------------------------- CLI, app
def test_cli_tol(gpu):
    cmd = [sys.executable, "-m", "cuda_mpi_scratch_amd.models.stencil2d", "--global", "48x32", "--non-periodic",
           "--block-fixed-edges", "--tol", "0.5", "--max-iters", "2000", "--warmup", "0"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=240, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    rec = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    st = Stencil2D(StencilConfig(global_width=48, global_height=32, dims="1x1", periodic=False,
                                 block_fixed_edges=True))
    want = st.run_until(0.5, 2000)
    assert want["converged"] and want["iterations"] > 0
    assert rec["converged"] is True and rec["iterations"] == want["iterations"] and rec["checks"] == want["checks"]
    assert rec["residual"] == want["residual"]


BIN = os.path.join(ROOT, "build", "bin")
MPIEXEC = shutil.which("mpiexec", path="/opt/conda/bin") or shutil.which("mpiexec")


@pytest.mark.skipif(not (MPIEXEC and os.path.exists(os.path.join(BIN, "stencil2d"))), reason="MPI GPU apps not built")
@pytest.mark.parametrize("warmup", [None, 0])
def test_app_tol(gpu, tmp_path, warmup):
    """One rank (local) and four ranks (mpi-staged) stop at the same iteration.
    With the app's default warm-up the field is below the tolerance at the
    first check; --warmup 0 makes both iterate."""
    args = ["--global", "48x32", "--non-periodic", "--block-fixed-edges", "--tol", "0.5", "--iters", "2000"]
    if warmup is not None:
        args += ["--warmup", str(warmup)]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    found = []
    for n, extra in ((1, []), (4, ["--backend", "mpi-staged"])):
        r = subprocess.run([MPIEXEC, "-n", str(n), os.path.join(BIN, "stencil2d"), *args, *extra],
                           capture_output=True, text=True, timeout=240, cwd=tmp_path, env=env)
        assert r.returncode == 0, r.stderr[-3000:]
        m = re.search(r"^converged after (\d+) iterations, residual ([0-9.eE+-]+) \(linf\)$", r.stdout, re.M)
        assert m, r.stdout[-2000:]
        rec = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
        assert rec["converged"] is True and rec["iterations"] == int(m.group(1)) and rec["checks"] >= 1
        found.append((int(m.group(1)), m.group(2)))
    assert found[0] == found[1]
    if warmup == 0:
        assert found[0][0] > 0
