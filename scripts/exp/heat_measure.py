"""Measurements of the implicit heat step for docs/PERF.md "Implicit heat steps"
(MI355X; every timing ends in a device synchronise or is taken with device
events, after a warm-up, as the median of REPS repetitions with min and max).

  step       time per step, fused native step() against the same step through the
             public solver API (field(), the right-hand side in torch, set_source,
             solve), same process, alternating
  start      the fused start kernel alone against a device right-hand-side pass
             (stencil5 with weights (a, b)) plus pcg_start / cg_start, device events
  crossover  time per step of cg and pcg over lam
  stiff      counts and time per step at lam = 1e4, backward Euler and Crank-Nicolson

    python scripts/exp/heat_measure.py step start crossover stiff [--out FILE]
"""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import torch  # noqa: E402

from cuda_mpi_scratch_amd import ops  # noqa: E402
from cuda_mpi_scratch_amd.models import HeatConfig, ImplicitHeat2D  # noqa: E402
from cuda_mpi_scratch_amd.models.pcg2d import MultigridPcg2D, PcgConfig  # noqa: E402

REPS = 5
OUT = None


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if OUT:
        with open(OUT, "a") as f:
            f.write(line + "\n")


def stats(ts):
    return {"median_s": statistics.median(ts), "min_s": min(ts), "max_s": max(ts), "reps": len(ts)}


def start_field(n):
    gen = torch.Generator(device="cpu").manual_seed(n)
    return torch.rand(n, n, generator=gen, dtype=torch.float64).cuda()


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def measure_step(n, lam=100.0, theta=1.0):
    u0 = start_field(n)
    tol = 1e-10 * float(torch.linalg.vector_norm(u0))
    h = ops.heat_coefficients(lam, theta)
    fused = ImplicitHeat2D(HeatConfig(width=n, height=n, lam=lam, theta=theta, method="pcg"), device="cuda")
    plain = MultigridPcg2D(PcgConfig(width=n, height=n, c_center=0.0, c_neighbor=h["c1"]), device="cuda")

    def unfused_step():
        full = plain.full()
        c = full[1:-1, 1:-1]
        g = h["a"] * c
        if h["b"] != 0.0:
            g = g + h["b"] * ((full[:-2, 1:-1] + full[2:, 1:-1]) + (full[1:-1, :-2] + full[1:-1, 2:]))
        plain.set_source(g)
        return plain.solve(tol)

    tf, tu, its = [], [], None
    for rep in range(REPS + 1):  # the first pair is the warm-up (graph capture, allocator)
        fused.set_field(u0)
        a, of = timed(lambda: fused.step(1, tol))
        plain.set_field(u0)
        b, ou = timed(unfused_step)
        assert of["converged"] and ou["converged"]
        its = (of["iterations"][0], ou["iterations"])
        if rep:
            tf.append(a)
            tu.append(b)
    diff = float(torch.linalg.vector_norm(fused.field() - plain.field()))
    emit({"what": "step", "size": n, "lam": lam, "theta": theta, "tol": tol, "iterations_fused_unfused": its,
          "fused": stats(tf), "unfused": stats(tu), "ratio_unfused_over_fused": statistics.median(tu) / statistics.median(tf),
          "field_difference_l2": diff, "D_tol": h["D"] * tol})


def events(fn, reps=20, warm=3):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e-3)
    return stats(ts)


def measure_start(n, lam=100.0, theta=0.5):
    dt = torch.float64
    m = MultigridPcg2D(PcgConfig(width=n, height=n, c_center=0.0, c_neighbor=0.2), device="cuda")
    g = m.geom
    del m
    h = ops.heat_coefficients(lam, theta)
    tiles = {k: torch.zeros(g.alloc_elems(), dtype=dt, device="cuda") for k in ("u", "q", "g", "r", "p")}
    tiles["u"].uniform_(0, 1)
    tiles["q"].uniform_(0, 1)
    for name, ws in (("pcg", ops.PcgWorkspace(g, "cuda")), ("cg", ops.CgWorkspace(g, "cuda"))):
        ws.write(tol=0.0, max_iters=5, norm="l2")
        u, q, gt, r, p = (tiles[k] for k in ("u", "q", "g", "r", "p"))
        if name == "pcg":
            fused_q = lambda: ops.pcg_heat_start(u, q, gt, r, g, lam, theta, ws)  # noqa: E731
            fused_0 = lambda: ops.pcg_heat_start(u, None, gt, r, g, lam, theta, ws)  # noqa: E731
            start = lambda: ops.pcg_start(u, gt, r, g, 0.0, h["c1"], ws)  # noqa: E731
        else:
            fused_q = lambda: ops.cg_heat_start(u, q, gt, r, p, g, lam, theta, ws)  # noqa: E731
            fused_0 = lambda: ops.cg_heat_start(u, None, gt, r, p, g, lam, theta, ws)  # noqa: E731
            start = lambda: ops.cg_start(u, gt, r, p, g, 0.0, h["c1"], ws)  # noqa: E731
        rhs = lambda: ops.stencil5(u, gt, g, 0, None, h["a"], h["b"])  # noqa: E731

        def unfused():
            rhs()
            start()

        emit({"what": "start", "kernel": name, "size": n, "fused_with_source": events(fused_q),
              "fused_no_source": events(fused_0), "rhs_pass_plus_start_no_source": events(unfused),
              "rhs_pass": events(rhs), "start": events(start),
              "arrays": {"fused_with_source": 4 if name == "pcg" else 5, "fused_no_source": 3 if name == "pcg" else 4,
                         "unfused_no_source": 5 if name == "pcg" else 6}})


def measure_method(n, lam, theta, method, what):
    u0 = start_field(n)
    tol = 1e-10 * float(torch.linalg.vector_norm(u0))
    m = ImplicitHeat2D(HeatConfig(width=n, height=n, lam=lam, theta=theta, method=method), device="cuda")
    ts, its = [], None
    for rep in range(REPS + 1):
        m.set_field(u0)
        t, out = timed(lambda: m.step(1, tol))
        assert out["converged"], out
        its = out["iterations"][0]
        if rep:
            ts.append(t)
    emit({"what": what, "size": n, "lam": lam, "theta": theta, "method": method, "iterations": its, "tol": tol,
          **stats(ts)})


def main(argv):
    global OUT
    if "--out" in argv:
        OUT = argv[argv.index("--out") + 1]
    assert torch.cuda.is_available(), "the measurements need the GPU"
    if "step" in argv:
        for n in (2048, 8192):
            measure_step(n)
    if "start" in argv:
        measure_start(8192)
    if "crossover" in argv:
        for lam in (0.25, 1.0, 4.0, 16.0, 64.0, 256.0):
            for method in ("cg", "pcg"):
                measure_method(2048, lam, 1.0, method, "crossover")
    if "stiff" in argv:
        for theta in (1.0, 0.5):
            measure_method(2048, 1e4, theta, "pcg", "stiff")
        # the Poisson solve the stiff step is compared with: same grid, same tolerance
        u0 = start_field(2048)
        tol = 1e-10 * float(torch.linalg.vector_norm(u0))
        p = MultigridPcg2D(PcgConfig(width=2048, height=2048), device="cuda")
        ts = []
        for rep in range(REPS + 1):
            p.set_field(u0)
            t, out = timed(lambda: p.solve(tol))
            if rep:
                ts.append(t)
        emit({"what": "poisson", "size": 2048, "iterations": out["iterations"], "converged": out["converged"], **stats(ts)})


if __name__ == "__main__":
    main(sys.argv[1:])
