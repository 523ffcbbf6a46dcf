"""Worker and launcher of the multi-rank residual / run_until tests
(tests/test_gpu_residual.py, tests/test_residual_cpu.py): one rank of a
non-periodic grid with fixed edges, on a shared GPU (native solver, IPC
backend) or on the CPU (torch backend), gloo rendezvous from RANK / WORLD_SIZE /
MASTER_ADDR / MASTER_PORT. Calls ``residual()`` and ``run_until(...)`` and prints
one ``RESULT `` JSON line; rank 0's carries the gathered global grid."""
import json
import os
import socket
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def boundary(w, h):
    """The fixed edges of the stopping-rule tests: hot top, cold bottom, a ramp
    on the left, 50 on the right."""
    import torch

    return dict(top=100.0, bottom=0.0, left=torch.linspace(100.0, 0.0, h, dtype=torch.float64), right=50.0)


def padded(core, bnd=None):
    """The (H + 2, W + 2) float64 view of a global core with its 1-deep ring:
    wrapped (periodic, ``bnd`` None) or the boundary values (corners unused)."""
    import torch

    u = core.double()
    if bnd is None:
        return torch.nn.functional.pad(u[None, None], (1, 1, 1, 1), mode="circular")[0, 0]
    p = torch.zeros(u.shape[0] + 2, u.shape[1] + 2, dtype=torch.float64)
    p[1:-1, 1:-1] = u
    p[0, 1:-1], p[-1, 1:-1], p[1:-1, 0], p[1:-1, -1] = bnd["top"], bnd["bottom"], bnd["left"], bnd["right"]
    return p


def reference_history(core0, every, checks, bnd=None, c_center=0.2, c_neighbor=0.2):
    """float64 CPU reference of run_until's checks: [(linf, l2)] of the residual
    at iterations 0, every, 2 * every, ... (`checks` entries), from the global
    core `core0` with wrapped or fixed edges."""
    from cuda_mpi_scratch_amd import ops

    u = core0.double().clone()
    hist = []
    for k in range(checks):
        hist.append(ops.residual5_reference(padded(u, bnd), 1, c_center, c_neighbor))
        if k + 1 < checks:
            for _ in range(every):
                p = padded(u, bnd)
                u = c_neighbor * ((p[:-2, 1:-1] + p[2:, 1:-1]) + (p[1:-1, :-2] + p[1:-1, 2:])) + c_center * u
    return hist


def main(args):
    sys.path.insert(0, ROOT)
    from cuda_mpi_scratch_amd.models.stencil2d import Stencil2D, StencilConfig
    from cuda_mpi_scratch_amd.parallel import init

    device = args.get("device", "cuda")
    ctx = init(backend="gloo", device=device)
    cfg = StencilConfig(global_width=args["w"], global_height=args["h"], dims=args["dims"],
                        dtype=args.get("dtype", "f32"), seed=args.get("seed", 5),
                        backend=args.get("backend", "ipc" if device == "cuda" else "torch"), periodic=False,
                        block_fixed_edges=True, time_block=args.get("time_block", 12), sum_form=False,
                        direct_halo=args.get("direct_halo", None))
    st = Stencil2D(cfg, ctx, device=device) if device == "cpu" else Stencil2D(cfg, ctx)
    st.set_boundary(**boundary(args["w"], args["h"]))
    first = st.residual()
    res = st.run_until(args["tol"], args["max_iters"], args.get("check_every", 0), args.get("norm", "linf"))
    st.synchronize()
    g = st.gather_global()
    out = {"rank": ctx.rank, "first": first, "until": res, "iteration": st.iteration,
           "direct": bool(st.solver.direct_halo()) if st.solver is not None else False}
    if ctx.rank == 0:
        out["grid"] = g.double().tolist()
    ctx.barrier()
    ctx.destroy()
    return out


# ------------------------------------------------------------------ launcher
class _PortTaken(RuntimeError):
    pass


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _launch_once(nprocs, args, timeout):
    port = _free_port()
    procs = []
    for r in range(nprocs):
        env = dict(os.environ)
        env.update(RANK=str(r), WORLD_SIZE=str(nprocs), LOCAL_RANK=str(r), LOCAL_WORLD_SIZE=str(nprocs),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), OMP_NUM_THREADS="1",
                   HSA_ENABLE_IPC_MODE_LEGACY="0")
        if args.get("device", "cuda") == "cpu":
            env.update(CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__), json.dumps(args)], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    results = []
    try:
        for p in procs:
            out, err = p.communicate(timeout=timeout)
            if p.returncode != 0:
                if "EADDRINUSE" in err or "address already in use" in err:
                    raise _PortTaken(err[-500:])
                raise RuntimeError(f"rank failed rc={p.returncode}\n{err[-3000:]}")
            line = [ln for ln in out.splitlines() if ln.startswith("RESULT ")]
            assert line, f"no result\nstdout={out[-2000:]}\nstderr={err[-2000:]}"
            results.append(json.loads(line[-1][len("RESULT "):]))
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
        for p in procs:
            try:
                p.wait(timeout=30)
            except subprocess.TimeoutExpired:
                pass
    return sorted(results, key=lambda r: r["rank"])


def launch(nprocs, args, timeout=180):
    """Run `nprocs` ranks of this worker; only a rendezvous port taken before
    rank 0 bound it (nothing ran yet) is retried."""
    for _ in range(3):
        try:
            return _launch_once(nprocs, args, timeout)
        except _PortTaken:
            continue
    return _launch_once(nprocs, args, timeout)


if __name__ == "__main__":
    result = main(json.loads(sys.argv[1]))
    sys.stdout.write("RESULT " + json.dumps(result) + "\n")
    sys.stdout.flush()
