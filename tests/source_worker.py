"""Worker and launcher of the multi-rank source-term tests
(tests/test_source_cpu.py, tests/test_gpu_source.py): one rank of a grid with
fixed edges and a source term, on a shared GPU (native solver, IPC backend) or
on the CPU (torch backend), gloo rendezvous from RANK / WORLD_SIZE /
MASTER_ADDR / MASTER_PORT. Builds the model, calls ``set_source``, runs
``run(n)`` for every n of ``runs`` (or ``run_until``), with an optional
checkpoint save / resume, and prints one ``RESULT `` JSON line; rank 0's
carries the gathered global grid as the hex of its bytes (bitwise comparisons)."""
import json
import os
import socket
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)

from tests.relaxation_worker import BOUNDARY  # noqa: E402

DTYPES = {"f32": "float32", "f64": "float64"}


def global_source(args):
    """The global ``g`` of a run: ``None``, a scalar, or a seeded random field in
    [-amp, amp] rounded to fp32 first (every precision sees the same data)."""
    import torch

    g = args.get("g", {"seed": 11, "amp": 0.01})
    if g is None or isinstance(g, (int, float)):
        return g
    gen = torch.Generator(device="cpu").manual_seed(int(g["seed"]))
    r = torch.rand(args["h"], args["w"], generator=gen, dtype=torch.float64)
    r = ((2.0 * r - 1.0) * float(g.get("amp", 0.01))).float()
    return r.to(getattr(torch, DTYPES[args.get("dtype", "f32")]))


def make(args, ctx=None, device=None, source=True):
    """The model of the tests: fixed edges BOUNDARY (``boundary="zero"``: 0), the
    seeded random start (``zero``: 0), ``source=True``."""
    from cuda_mpi_scratch_amd.models.stencil2d import Stencil2D, StencilConfig

    device = device or args.get("device", "cuda")
    cfg = StencilConfig(global_width=args["w"], global_height=args["h"], dims=args.get("dims", "1x1"),
                        dtype=args.get("dtype", "f32"), seed=args.get("seed", 5),
                        backend=args.get("backend", "auto" if device == "cuda" else "torch"), periodic=False,
                        block_fixed_edges=True, time_block=args.get("time_block", 20), sum_form=False,
                        graph=args.get("graph", True), relaxation=args.get("relaxation", "chebyshev"), source=source)
    st = Stencil2D(cfg, ctx, device=device) if device == "cpu" else Stencil2D(cfg, ctx)
    if args.get("zero", False):
        st.a.zero_()
        st.b.zero_()
    if args.get("boundary", "issue") == "zero":
        st.set_boundary(top=0.0, bottom=0.0, left=0.0, right=0.0)
    else:
        st.set_boundary(**BOUNDARY)
    return st


def main(args):
    from cuda_mpi_scratch_amd.parallel import init

    device = args.get("device", "cuda")
    ctx = init(backend="gloo", device=device)
    st = make(args, ctx, device)
    if args.get("resume"):
        st.load_checkpoint(args["resume"])
    st.set_source(global_source(args))
    until = None
    for i, n in enumerate(args.get("runs", [])):
        st.run(n)
        if args.get("save") and i == args.get("save_after", 0):
            st.synchronize()
            st.save_checkpoint(args["save"])
    if "tol" in args:
        until = st.run_until(args["tol"], args["max_iters"], args.get("check_every", 0), args.get("norm", "linf"))
    res = st.residual()
    st.synchronize()
    g = st.gather_global()
    out = {"rank": ctx.rank, "iteration": st.iteration, "until": until, "note": st.relaxation_note(),
           "cycle": st.cycle, "time_block": st.time_block, "residual": res}
    if ctx.rank == 0:
        out["grid"] = g.contiguous().numpy().tobytes().hex()
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
