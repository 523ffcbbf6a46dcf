"""Measurements of the conjugate-gradient solver (profiles/cg). One JSON line per
measurement into OUT, each with the box's name.

    python scripts/exp/cg_measure.py OUT [iteration] [load[=SIZE]] [chebyshev[=SIZE]] [multigrid[=SIZE]]

iteration : time per CG iteration at 2048^2, 4096^2 and 8192^2, fp32 and fp64,
            graph and eager: windows of ITERS iterations (host clock around
            solve(0, ITERS, check_every=ITERS): one cg_start, ITERS iterations
            with no host check in between, one read of the scalars and one true
            residual, 6 array streams against the window's 10 ITERS), REPEATS
            windows after one untimed window; the median against the byte model
            10 W H sizeof(T) and the 5.3 TB/s copy roof.
load      : the README's constant load (f = 1 on the unit square, g = 0.2 h^2,
            zero boundary and start) in fp64 at SIZE (default 2048): iterations
            and wall time of solve(1e-8, norm="l2"), median of REPEATS solves
            from the same start.
chebyshev : the same problem at SIZE with the relaxation solver
            (multigrid_measure.chebyshev), in the same call.
multigrid : the same problem at SIZE (default 2047) with Multigrid2D
            (multigrid_measure.poisson) and with CG, in the same call.
"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

import multigrid_measure as mgm  # noqa: E402
from cuda_mpi_scratch_amd.models.cg2d import CgConfig, ConjugateGradient2D  # noqa: E402

SIZES = (2048, 4096, 8192)
ITERS = 200
REPEATS = 5
ROOF_TBS = 5.3
MODEL_ARRAYS = 10.0
TOL = 1e-8


def iteration(out):
    for n in SIZES:
        for dtype in ("f32", "f64"):
            for graph in (True, False):
                m = ConjugateGradient2D(CgConfig(width=n, height=n, dtype=dtype, graph=graph, check_every=ITERS),
                                        device="cuda")
                m.set_boundary(top=1.0)
                m.set_source(1e-6)
                res = m.solve(0.0, ITERS)  # untimed: capture, first launches, sustained clocks
                ms = []
                for _ in range(REPEATS):
                    m.set_field(0.0)
                    t0 = time.perf_counter()
                    res = m.solve(0.0, ITERS)
                    ms.append((time.perf_counter() - t0) * 1e3 / ITERS)
                assert res["iterations"] == ITERS, res
                med = statistics.median(ms)
                model_bytes = MODEL_ARRAYS * n * n * (4 if dtype == "f32" else 8)
                mgm.emit(out, {"measure": "iteration", "size": f"{n}x{n}", "dtype": dtype, "graph": m.graph_status(),
                               "iterations_per_window": ITERS, "windows": REPEATS, "ms_per_iteration": med,
                               "ms_min": min(ms), "ms_max": max(ms), "model_bytes": model_bytes,
                               "model_tb_s": model_bytes / med / 1e9, "roof_fraction": model_bytes / med / 1e9 / ROOF_TBS,
                               "note": m.note()})
                del m
                torch.cuda.empty_cache()


def load(out, n):
    _, g, a = mgm.poisson_problem(n, "load")
    m = ConjugateGradient2D(CgConfig(width=n, height=n, dtype="f64"), device="cuda")
    m.set_source(g)
    m.solve(TOL, 64)  # capture and first launches outside the timed solves
    wall, res = [], None
    for _ in range(REPEATS):
        m.set_field(0.0)
        t0 = time.perf_counter()
        res = m.solve(TOL, 100000, "l2")
        wall.append(time.perf_counter() - t0)
    u = m.field().cpu()
    mgm.emit(out, {"measure": "cg", "problem": "load", "max_u": float(u.max()), "size": f"{n}x{n}", "dtype": "f64",
                   "tol": TOL, "norm": "l2", "converged": res["converged"], "iterations": res["iterations"],
                   "restarts": res["restarts"], "reason": res["reason"], "residual": res["residual"],
                   "recursive_l2": res["history"][-1][2], "checks": len(res["history"]),
                   "wall_s": statistics.median(wall), "wall_min_s": min(wall), "wall_max_s": max(wall),
                   "bound": TOL / a, "note": m.note()})
    del m
    torch.cuda.empty_cache()


if __name__ == "__main__":
    out = sys.argv[1]
    assert torch.cuda.is_available(), "measurements need the GPU"
    for w in sys.argv[2:] or ["iteration", "load", "chebyshev", "multigrid"]:
        name, _, arg = w.partition("=")
        if name == "iteration":
            iteration(out)
        elif name == "load":
            load(out, int(arg) if arg else 2048)
        elif name == "chebyshev":
            mgm.chebyshev(out, int(arg) if arg else 2048, "load")
        elif name == "multigrid":
            n = int(arg) if arg else 2047
            mgm.poisson(out, sizes=(n,), problem="load")
            load(out, n)
        else:
            raise SystemExit(f"unknown measurement {w!r}")
