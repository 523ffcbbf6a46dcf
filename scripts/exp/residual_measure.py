"""Measurements of the residual norm and of run_until's checking overhead
(profiles/residual). One JSON line per measurement into OUT.

    python scripts/exp/residual_measure.py OUT [kernel] [overhead]

kernel   : event-timed (stencil5_residual, absmax) launch pairs over one tile
           in one process, after a warm-up burst; medians, the read rate over
           the core's bytes (residual) and over the buffer's bytes (absmax).
overhead : one fused periodic solver per size; paired rounds of plain run(960)
           and run_until(tol=0, max_iters=960) at check_every = 8, 16 and 32
           time blocks (16 is the default), each from the same restored field with streams drained
           (host clock around work that ends in a synchronise); medians of the
           per-round ratios.
"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from cuda_mpi_scratch_amd import core, hip  # noqa: E402
from cuda_mpi_scratch_amd.models.stencil2d import Stencil2D, StencilConfig  # noqa: E402

ITERS = 960
ROUNDS = 9


def emit(out, rec):
    line = json.dumps(rec)
    print(line, flush=True)
    with open(out, "a") as f:
        f.write(line + "\n")


def kernel(out):
    H = hip()
    for w, h, dtype, ring in ((8192, 8192, "f32", 24), (32768, 32768, "f32", 24), (8192, 8192, "f64", 16)):
        tdt = torch.float32 if dtype == "f32" else torch.float64
        es = 4 if dtype == "f32" else 8
        g = core().TileGeom.aligned(w, h, ring, ring, es)
        buf = torch.rand(g.alloc_elems(), dtype=tdt, device="cuda")
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < 1.0:  # sustained clocks before the timed pairs
            H.residual_kernel_times(buf.data_ptr(), g, 0.2, 0.2, dtype, 10)
        r = H.residual_kernel_times(buf.data_ptr(), g, 0.2, 0.2, dtype, 40)
        res_ms, abs_ms = statistics.median(r["residual_ms"]), statistics.median(r["absmax_ms"])
        core_bytes, buf_bytes = w * h * es, g.alloc_elems() * es
        emit(out, {"measure": "kernel", "size": f"{w}x{h}", "dtype": dtype, "ring": ring, "pairs": 40,
                   "workgroups": r["workgroups"], "residual_ms": res_ms, "residual_ms_min": min(r["residual_ms"]),
                   "residual_ms_max": max(r["residual_ms"]), "absmax_ms": abs_ms,
                   "absmax_ms_min": min(r["absmax_ms"]), "absmax_ms_max": max(r["absmax_ms"]),
                   "core_bytes": core_bytes, "buffer_bytes": buf_bytes,
                   "residual_gbs_core": core_bytes / res_ms / 1e6, "absmax_gbs_buffer": buf_bytes / abs_ms / 1e6,
                   "rate_ratio": (core_bytes / res_ms) / (buf_bytes / abs_ms),
                   "raw_residual_ms": r["residual_ms"], "raw_absmax_ms": r["absmax_ms"]})
        del buf
        torch.cuda.empty_cache()


def overhead(out):
    for w, h in ((8192, 8192), (32768, 32768)):
        st = Stencil2D(StencilConfig(global_width=w, global_height=h, dims="1x1", dtype="f32"))
        tb = st.time_block
        start = st.a.clone()
        kinds = [("run", 0)] + [(f"until_{k}", k * tb) for k in (8, 16, 32)]
        for _, every in kinds:
            st.prepare(every or ITERS)
        st.prepare(ITERS)
        st.warm(ITERS, 1.0)
        st.residual()

        def window(every):
            # The same field every time; the first run after a field change
            # re-measures the sum form's range, so one untimed pass absorbs it.
            cur = st.current()
            cur.copy_(start)
            st.run(tb)
            st.synchronize()
            t0 = time.perf_counter()
            if every:
                res = st.run_until(0.0, ITERS, every)
                assert res["iterations"] == ITERS and not res["converged"], res
                checks = res["checks"]
            else:
                st.run(ITERS)
                checks = 0
            st.synchronize()
            return time.perf_counter() - t0, checks

        times = {name: [] for name, _ in kinds}
        checks = {}
        for _ in range(ROUNDS):
            for name, every in kinds:
                dt, checks[name] = window(every)
                times[name].append(dt * 1e3)
        base = times["run"]
        rec = {"measure": "overhead", "size": f"{w}x{h}", "dtype": "f32", "time_block": tb, "iters": ITERS,
               "rounds": ROUNDS, "run_ms": statistics.median(base),
               "run_tcells_s": w * h * ITERS / statistics.median(base) / 1e9, "raw_ms": times}
        for name, every in kinds[1:]:
            ratios = [a / b for a, b in zip(times[name], base)]
            rec[name] = {"check_every": every, "checks": checks[name], "ms": statistics.median(times[name]),
                         "ratio_median": statistics.median(ratios), "ratio_min": min(ratios),
                         "ratio_max": max(ratios)}
        emit(out, rec)
        del st, start
        torch.cuda.empty_cache()


if __name__ == "__main__":
    out = sys.argv[1]
    what = sys.argv[2:] or ["kernel", "overhead"]
    assert torch.cuda.is_available(), "measurements need the GPU"
    if "kernel" in what:
        kernel(out)
    if "overhead" in what:
        overhead(out)
