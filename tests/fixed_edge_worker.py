"""Worker of tests/test_gpu_fixed_edges.py: one rank of a non-periodic grid on a
shared GPU (gloo rendezvous, RANK / WORLD_SIZE / MASTER_ADDR / MASTER_PORT from
the launcher). Runs the native solver with or without time blocking beside the
fixed edges and prints one ``RESULT `` JSON line; rank 0's carries the gathered
global grid."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cuda_mpi_scratch_amd.models.stencil2d import Stencil2D, StencilConfig  # noqa: E402
from cuda_mpi_scratch_amd.parallel import init  # noqa: E402


def main(args):
    ctx = init(backend="gloo", device="cuda")
    cfg = StencilConfig(global_width=args["w"], global_height=args["h"], dims=args["dims"],
                        dtype=args.get("dtype", "f32"), seed=args.get("seed", 5), backend=args.get("backend", "ipc"),
                        periodic=False, block_fixed_edges=bool(args.get("block_fixed_edges", False)),
                        time_block=args.get("time_block", 12), sum_form=False,
                        direct_halo=args.get("direct_halo", False))
    st = Stencil2D(cfg, ctx)
    openings = []
    for n in args["runs"]:
        st.run(n)
        openings.append(st.solver.last_run_opening())
    st.synchronize()
    g = st.gather_global()
    out = {"rank": ctx.rank, "time_block": st.time_block, "openings": openings, "note": st.fixed_edge_note(),
           "held": int(st.solver.held_sides()), "direct": bool(st.solver.direct_halo()),
           "choice": st.solver.schedule_times()["opening"], "reason": st.solver.schedule_times()["reason"],
           "graph": st.graph_status()}
    if ctx.rank == 0:
        out["grid"] = g.double().tolist()
    ctx.barrier()
    ctx.destroy()
    return out


if __name__ == "__main__":
    res = main(json.loads(sys.argv[1]))
    sys.stdout.write("RESULT " + json.dumps(res) + "\n")
    sys.stdout.flush()
