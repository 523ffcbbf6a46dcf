"""Measurements of the multigrid-preconditioned CG solver (profiles/pcg). One
JSON line per measurement into OUT, each with the box's name.

    python scripts/exp/pcg_measure.py OUT
    python scripts/exp/pcg_measure.py OUT neumann      (profiles/neumann)

solve : the README's load (f = 1 on the unit square, g = c_neighbor h^2, zero
        boundary and start) in fp64 to l2 <= 1e-8: wall time (host clock around
        solve(), which ends in a synchronising read) and iterations, the median
        of REPEATS solves from the same start after one untimed solve, with the
        comparator interleaved solve by solve in the same process:
        2048^2 against ConjugateGradient2D, 2047^2 against Multigrid2D,
        3000 x 1000 and a screened 2048^2 (0.1999, 0.2) on their own.
split : the time of one iteration at 2048^2: ITERS iterations with tol = 0
        (max_iters = ITERS, one graph launch per 2) for the preconditioned
        solver and for plain CG, whose two kernels are the bodies of pcg_apply
        and pcg_update; the V-cycle's share is the difference.
neumann : the solve load at 2048^2 for MultigridPcg2D and ConjugateGradient2D
        with no Neumann side and with the left and the right side insulated,
        the four solvers interleaved solve by solve in one process; then the
        time of one iteration of each (the split's recipe). The no-Neumann
        figures are the ones to hold against profiles/pcg.
"""
import json
import os
import socket
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from cuda_mpi_scratch_amd.models.cg2d import CgConfig, ConjugateGradient2D  # noqa: E402
from cuda_mpi_scratch_amd.models.multigrid2d import Multigrid2D, MultigridConfig  # noqa: E402
from cuda_mpi_scratch_amd.models.pcg2d import MultigridPcg2D, PcgConfig  # noqa: E402

REPEATS = 5
ITERS = 40
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


def load(m, w, c1):
    m.set_boundary(top=0.0, bottom=0.0, left=0.0, right=0.0)
    m.set_source(c1 / float(w + 1) ** 2)
    m.set_field(0.0)


def timed_solve(m, **kw):
    m.set_field(0.0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = m.solve(TOL, **kw)
    return time.perf_counter() - t0, out


def stats(ts):
    return {"median_s": statistics.median(ts), "min_s": min(ts), "max_s": max(ts), "runs": len(ts)}


def solve_case(out, name, w, h, c0, c1, other):
    solvers = {"pcg": (MultigridPcg2D(PcgConfig(width=w, height=h, dtype="f64", c_center=c0, c_neighbor=c1),
                                      device="cuda"), {"max_iters": 1000})}
    if other == "cg":
        solvers["cg"] = (ConjugateGradient2D(CgConfig(width=w, height=h, dtype="f64", c_center=c0, c_neighbor=c1),
                                             device="cuda"), {"max_iters": 100000})
    elif other == "multigrid":
        solvers["multigrid"] = (Multigrid2D(MultigridConfig(width=w, height=h, dtype="f64"), device="cuda"),
                                {"max_cycles": 50})
    times, last = {k: [] for k in solvers}, {}
    for m, _ in solvers.values():
        load(m, w, c1)
    for rep in range(REPEATS + 1):  # the first round is untimed (capture, first touch)
        for k, (m, kw) in solvers.items():
            dt, res = timed_solve(m, **kw)
            last[k] = res
            if rep:
                times[k].append(dt)
    for k, (m, _) in solvers.items():
        res = last[k]
        emit(out, dict(stats(times[k]), kind="solve", case=name, solver=k, width=w, height=h, c_center=c0,
                       c_neighbor=c1, tol=TOL, converged=res["converged"], residual=res["residual"],
                       iterations=res.get("iterations", res.get("cycles")), reason=res["reason"], note=m.note()))
    if len(solvers) == 2:
        a, b = (statistics.median(times[k]) for k in solvers)
        emit(out, {"kind": "ratio", "case": name, "pcg_over_" + other: a / b, other + "_over_pcg": b / a})


def split_case(out, w, h):
    ms = {"pcg": MultigridPcg2D(PcgConfig(width=w, height=h, dtype="f64"), device="cuda"),
          "cg": ConjugateGradient2D(CgConfig(width=w, height=h, dtype="f64", check_every=2), device="cuda")}
    per = {k: [] for k in ms}
    for m in ms.values():
        load(m, w, 0.2)
    for rep in range(REPEATS + 1):
        for k, m in ms.items():
            m.set_field(0.0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = m.solve(0.0, ITERS, check_every=2)
            dt = time.perf_counter() - t0
            assert res["iterations"] == ITERS, res
            if rep:
                per[k].append(dt / ITERS)
    p, c = statistics.median(per["pcg"]), statistics.median(per["cg"])
    model = 24.0 * w * h * 8
    emit(out, {"kind": "split", "width": w, "height": h, "iterations": ITERS, "pcg_iteration_s": p,
               "apply_update_s": c, "vcycle_s": p - c, "vcycle_share": (p - c) / p,
               "pcg_iteration_min_s": min(per["pcg"]), "pcg_iteration_max_s": max(per["pcg"]),
               "byte_model_bytes": model, "byte_model_tb_s": model / p / 1e12,
               "launches_per_iteration": ms["pcg"].solver.launches_per_iteration()})


def neumann_case(out, w, h):
    sides = {"dirichlet": (), "neumann_left_right": ("left", "right")}
    ms = {}
    for tag, nm in sides.items():
        ms["pcg " + tag] = (MultigridPcg2D(PcgConfig(width=w, height=h, dtype="f64", neumann=nm), device="cuda"),
                            {"max_iters": 1000}, nm)
        ms["cg " + tag] = (ConjugateGradient2D(CgConfig(width=w, height=h, dtype="f64", neumann=nm), device="cuda"),
                           {"max_iters": 100000}, nm)
    for m, _, _ in ms.values():
        load(m, w, 0.2)
    times, last = {k: [] for k in ms}, {}
    for rep in range(REPEATS + 1):  # the first round is untimed (capture, first touch)
        for k, (m, kw, _) in ms.items():
            dt, res = timed_solve(m, **kw)
            last[k] = res
            if rep:
                times[k].append(dt)
    per = {k: [] for k in ms}
    for rep in range(REPEATS + 1):
        for k, (m, _, _) in ms.items():
            m.set_field(0.0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = m.solve(0.0, ITERS, check_every=2)
            dt = time.perf_counter() - t0
            assert res["iterations"] == ITERS, res
            if rep:
                per[k].append(dt / ITERS)
    for k, (m, _, nm) in ms.items():
        res = last[k]
        emit(out, dict(stats(times[k]), kind="neumann", solver=k.split()[0], neumann=list(nm), width=w, height=h,
                       tol=TOL, converged=res["converged"], residual=res["residual"], iterations=res["iterations"],
                       reason=res["reason"], iteration_median_s=statistics.median(per[k]),
                       iteration_min_s=min(per[k]), iteration_max_s=max(per[k]), note=m.note()))


def main():
    out = sys.argv[1]
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    if len(sys.argv) > 2 and sys.argv[2] == "neumann":
        neumann_case(out, 2048, 2048)
        return
    solve_case(out, "2048^2 vs CG", 2048, 2048, 0.2, 0.2, "cg")
    solve_case(out, "2047^2 vs multigrid", 2047, 2047, 0.2, 0.2, "multigrid")
    solve_case(out, "3000x1000", 3000, 1000, 0.2, 0.2, None)
    solve_case(out, "2048^2 screened", 2048, 2048, 0.1999, 0.2, None)
    split_case(out, 2048, 2048)


if __name__ == "__main__":
    main()
