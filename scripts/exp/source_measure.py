"""Measurements of the source term (profiles/source_term). One JSON line per
measurement into OUT.

    python scripts/exp/source_measure.py OUT [cost] [poisson]

cost    : what the correction's read stream costs. 8192^2 with fixed edges and
          Chebyshev cycles, fp32 M = 24 and fp64 M = 16: one solver, paired,
          alternating windows of 10 cycles with set_source(g) and with
          set_source(None) (host clock around work that ends in a synchronise,
          each window behind prepare() and one untimed window of its own
          kind); the per-pair ratios, their median and spread.
poisson : the manufactured problem (u* = sin sin, g = (1 - lambda) u*, zero
          boundary and start) at 2048^2 in fp64: iterations and wall time of
          run_until(1e-8, cap, norm="l2") with Chebyshev cycles (cap: 3 M
          iterations) and, capped at the sweeps Chebyshev needed, with the
          uniform table (plain Jacobi).
"""
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from cuda_mpi_scratch_amd.models.stencil2d import Stencil2D, StencilConfig  # noqa: E402

PAIRS = 8
CYCLES = 10


def emit(out, rec):
    line = json.dumps(rec)
    print(line, flush=True)
    with open(out, "a") as f:
        f.write(line + "\n")


def model(w, h, dtype, M, relaxation="chebyshev"):
    st = Stencil2D(StencilConfig(global_width=w, global_height=h, dims="1x1", dtype=dtype, periodic=False,
                                 block_fixed_edges=True, time_block=M, sum_form=False, relaxation=relaxation,
                                 source=True))
    st.a.zero_()
    st.b.zero_()
    return st


def cost(out):
    for dtype, M in (("f32", 24), ("f64", 16)):
        w = h = 8192
        st = model(w, h, dtype, M)
        st.set_boundary(top=100.0, bottom=0.0, left=0.0, right=50.0)
        gen = torch.Generator(device="cpu").manual_seed(1)
        g = ((torch.rand(h, w, generator=gen) * 2 - 1) * 0.01).to(st.dtype)
        n = CYCLES * M

        def window(with_source):
            st.set_source(g if with_source else None)
            st.prepare(n)
            st.run(n)  # untimed: this kind's kernels last on the device
            st.synchronize()
            t0 = time.perf_counter()
            st.run(n)
            st.synchronize()
            return (time.perf_counter() - t0) * 1e3

        window(True), window(False)  # sustained clocks, first launches
        src_ms, hom_ms = [], []
        for _ in range(PAIRS):
            src_ms.append(window(True))
            hom_ms.append(window(False))
        ratios = [a / b for a, b in zip(src_ms, hom_ms)]
        emit(out, {"measure": "cost", "size": f"{w}x{h}", "dtype": dtype, "cycle": M, "cycles_per_window": CYCLES,
                   "pairs": PAIRS, "ratio_median": statistics.median(ratios), "ratio_min": min(ratios),
                   "ratio_max": max(ratios), "source_ms": statistics.median(src_ms),
                   "homogeneous_ms": statistics.median(hom_ms),
                   "homogeneous_tcells_s": w * h * n / statistics.median(hom_ms) / 1e9,
                   "source_tcells_s": w * h * n / statistics.median(src_ms) / 1e9,
                   "note": st.relaxation_note(), "fixed_edges": st.fixed_edge_note(), "graph": st.graph_status(),
                   "raw_source_ms": src_ms, "raw_homogeneous_ms": hom_ms})
        del st, g
        torch.cuda.empty_cache()


def poisson(out):
    w = h = 2048
    M = 16
    i = torch.arange(1, w + 1, dtype=torch.float64)
    j = torch.arange(1, h + 1, dtype=torch.float64)
    u_star = torch.sin(j * math.pi / (h + 1))[:, None] * torch.sin(i * math.pi / (w + 1))[None, :]
    a = 1.0 - (0.2 + 0.4 * (math.cos(math.pi / (w + 1)) + math.cos(math.pi / (h + 1))))
    g = a * u_star
    cap = None
    for relaxation in ("chebyshev", "none"):
        st = model(w, h, "f64", M, relaxation)
        st.set_boundary(top=0.0, bottom=0.0, left=0.0, right=0.0)
        st.set_source(g)
        limit = cap or 3000000 // M * M
        st.prepare(16 * M)
        st.synchronize()
        t0 = time.perf_counter()
        res = st.run_until(1e-8, limit, norm="l2")
        st.synchronize()
        dt = time.perf_counter() - t0
        err = float(torch.linalg.vector_norm(st.core_view().cpu() - u_star))
        emit(out, {"measure": "poisson", "size": f"{w}x{h}", "dtype": "f64", "cycle": M, "relaxation": relaxation,
                   "tol": 1e-8, "norm": "l2", "cap": limit, "converged": res["converged"], "iterations": res["iterations"],
                   "residual": res["residual"], "checks": res["checks"], "wall_s": dt, "error_l2": err,
                   "bound": 1e-8 / a, "note": st.relaxation_note()})
        if relaxation == "chebyshev":
            cap = max(M, res["iterations"])  # the same number of sweeps
        del st
        torch.cuda.empty_cache()


if __name__ == "__main__":
    out = sys.argv[1]
    what = sys.argv[2:] or ["cost", "poisson"]
    assert torch.cuda.is_available(), "measurements need the GPU"
    if "cost" in what:
        cost(out)
    if "poisson" in what:
        poisson(out)
