"""Measurements of the multigrid solver (profiles/multigrid). One JSON line per
measurement into OUT, each with the box's name.

    python scripts/exp/multigrid_measure.py OUT [cycle] [poisson[-load]] [chebyshev[-load][=SIZE]] [reference[-load][=SIZES]]

cycle     : time per V(2,2) cycle at 2047^2, 4095^2 and 8191^2, fp32 and fp64,
            graph and eager: windows of CYCLES cycles (host clock around
            vcycle(n), which ends in a synchronise), REPEATS windows after one
            untimed window; the median against the byte model 14 W H sizeof(T)
            (per level: two smoother launches move 3 arrays each, restriction
            and prolongation 2 1/4 each = 10.5, x 4/3 over the levels) and the
            5.3 TB/s copy roof.
poisson   : the manufactured Poisson problem of docs/PERF.md "Source term" (u* =
            sin sin, g = (1 - lambda) u*, zero boundary and start) in fp64 at the
            three sizes: cycles and wall time
            of solve(1e-8, norm="l2") (median of REPEATS solves from the same
            start), the error against u* and its bound.
chebyshev : the same problem at SIZE (default 2047) with the relaxation solver:
            Stencil2D(relaxation="chebyshev", source=True).run_until(1e-8,
            norm="l2"), iterations and wall time.
reference : the pure-torch reference's cycle counts for the poisson problem on
            the CPU at SIZES (default 2047; needs no GPU, minutes per size).
poisson-load, chebyshev-load, reference-load : the same three with the README's
            constant load instead (f = 1 on the unit square, g = 0.2 h^2, zero
            boundary and start).
"""
import json
import math
import os
import socket
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from cuda_mpi_scratch_amd.models.multigrid2d import Multigrid2D, MultigridConfig  # noqa: E402

SIZES = (2047, 4095, 8191)
CYCLES = 20
REPEATS = 5
ROOF_TBS = 5.3
MODEL_ARRAYS = 14.0
TOL = 1e-8


def box():
    name = socket.gethostname()
    if torch.cuda.is_available():
        name += " / " + torch.cuda.get_device_name(0)
    return name


def emit(out, rec):
    rec = dict(rec, box=box())
    line = json.dumps(rec)
    print(line, flush=True)
    with open(out, "a") as f:
        f.write(line + "\n")


def poisson_problem(n, problem="manufactured"):
    """(u* or None, g, a): the manufactured problem, or the README's constant load
    f = 1 on the unit square (g = 0.2 h^2, h = 1 / (n + 1); no closed form)."""
    a = 1.0 - (0.2 + 0.8 * math.cos(math.pi / (n + 1)))
    if problem == "load":
        h = 1.0 / (n + 1)
        return None, 0.2 * h * h * torch.ones(n, n, dtype=torch.float64), a
    i = torch.arange(1, n + 1, dtype=torch.float64)
    s = torch.sin(i * math.pi / (n + 1))
    u_star = s[:, None] * s[None, :]
    return u_star, a * u_star, a


def cycle(out):
    for n in SIZES:
        for dtype in ("f32", "f64"):
            for graph in (True, False):
                m = Multigrid2D(MultigridConfig(width=n, height=n, dtype=dtype, graph=graph), device="cuda")
                m.set_boundary(top=1.0)
                m.set_source(1e-6)
                m.vcycle(CYCLES)  # untimed: capture, first launches, sustained clocks
                ms = []
                for _ in range(REPEATS):
                    t0 = time.perf_counter()
                    m.vcycle(CYCLES)
                    ms.append((time.perf_counter() - t0) * 1e3 / CYCLES)
                med = statistics.median(ms)
                model_bytes = MODEL_ARRAYS * n * n * (4 if dtype == "f32" else 8)
                emit(out, {"measure": "cycle", "size": f"{n}x{n}", "dtype": dtype, "graph": m.graph_status(),
                           "cycles_per_window": CYCLES, "windows": REPEATS, "ms_per_cycle": med, "ms_min": min(ms),
                           "ms_max": max(ms), "model_bytes": model_bytes, "model_tb_s": model_bytes / med / 1e9,
                           "roof_fraction": model_bytes / med / 1e9 / ROOF_TBS,
                           "launches_per_cycle": m.solver.launches_per_cycle(), "note": m.note()})
                del m
                torch.cuda.empty_cache()


def poisson(out, device="cuda", sizes=SIZES, problem="manufactured"):
    for n in sizes:
        u_star, g, a = poisson_problem(n, problem)
        m = Multigrid2D(MultigridConfig(width=n, height=n, dtype="f64"), device=device)
        m.set_source(g)
        if device == "cuda":
            m.vcycle(1)  # capture and first launches outside the timed solves
        wall, res = [], None
        for _ in range(REPEATS if device == "cuda" else 1):
            m.set_field(0.0)
            t0 = time.perf_counter()
            res = m.solve(TOL, 50, "l2")
            wall.append(time.perf_counter() - t0)
        u = m.field().cpu()
        err = float(torch.linalg.vector_norm(u - u_star)) if u_star is not None else None
        emit(out, {"measure": "poisson" if device == "cuda" else "reference", "problem": problem, "max_u": float(u.max()),
                   "size": f"{n}x{n}", "dtype": "f64", "device": device, "tol": TOL, "norm": "l2", "converged": res["converged"], "cycles": res["cycles"],
                   "reason": res["reason"], "residual": res["residual"], "wall_s": statistics.median(wall),
                   "wall_min_s": min(wall), "wall_max_s": max(wall), "sweep_equivalents": m.sweep_equivalents(res["cycles"]),
                   "error_l2": err, "bound": TOL / a, "l2_history": [h[2] for h in res["history"]], "note": m.note()})
        del m
        if device == "cuda":
            torch.cuda.empty_cache()


def chebyshev(out, n, problem="manufactured"):
    from cuda_mpi_scratch_amd.models.stencil2d import Stencil2D, StencilConfig

    M = 16
    u_star, g, a = poisson_problem(n, problem)
    st = Stencil2D(StencilConfig(global_width=n, global_height=n, dims="1x1", dtype="f64", periodic=False,
                                 block_fixed_edges=True, time_block=M, sum_form=False, relaxation="chebyshev",
                                 source=True))
    st.a.zero_()
    st.b.zero_()
    st.set_boundary(top=0.0, bottom=0.0, left=0.0, right=0.0)
    st.set_source(g)
    st.prepare(16 * M)
    st.synchronize()
    t0 = time.perf_counter()
    res = st.run_until(TOL, 3000000 // M * M, norm="l2")
    st.synchronize()
    dt = time.perf_counter() - t0
    u = st.core_view().cpu()
    err = float(torch.linalg.vector_norm(u - u_star)) if u_star is not None else None
    emit(out, {"measure": "chebyshev", "problem": problem, "max_u": float(u.max()), "size": f"{n}x{n}", "dtype": "f64",
               "cycle": M, "tol": TOL, "norm": "l2", "converged": res["converged"], "iterations": res["iterations"], "residual": res["residual"],
               "checks": res["checks"], "wall_s": dt, "error_l2": err, "bound": TOL / a, "note": st.relaxation_note(),
               "fixed_edges": st.fixed_edge_note()})


if __name__ == "__main__":
    out = sys.argv[1]
    what = sys.argv[2:] or ["cycle", "poisson", "chebyshev"]
    for w in what:
        name, _, arg = w.partition("=")
        problem = "manufactured"
        if name.endswith("-load"):  # poisson-load, chebyshev-load, reference-load: the constant load
            name, problem = name[:-5], "load"
        if name == "reference":
            poisson(out, "cpu", tuple(int(s) for s in arg.split(",")) if arg else (2047,), problem)
            continue
        assert torch.cuda.is_available(), "measurements need the GPU"
        if name == "cycle":
            cycle(out)
        elif name == "poisson":
            poisson(out, problem=problem)
        elif name == "chebyshev":
            chebyshev(out, int(arg) if arg else 2047, problem)
        else:
            raise SystemExit(f"unknown measurement {w!r}")
