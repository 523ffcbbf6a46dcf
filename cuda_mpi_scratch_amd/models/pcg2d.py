"""Multigrid-preconditioned conjugate gradients: the fast fixed-edge Poisson solve
``u = A u + g`` for any grid size.

``A u = c0 u + c1 (n + s + w + e)`` on a ``W x H`` core whose depth-1 ring holds
the Dirichlet values; any weights with ``c1 > 0`` and ``c0 + 4 c1 <= 1`` and any
sides but very thin ones (halving both axes together must end at most 63 on a
side; the error names ``ConjugateGradient2D`` otherwise). CG is preconditioned by
one V(nu, nu) cycle whose coarsening takes even sides through a reflecting ghost
(docs/ARCHITECTURE.md "Preconditioned CG"), so the iteration count stays near 10
where plain CG needs thousands. On a GPU ``MultigridPcg2D`` drives the native
``PcgSolver`` (HIP kernels, the dot products fused in, a linear captured hipGraph
per ``check_every`` iterations, the stopping test on the device); on the CPU it
runs the pure-torch references of ``ops.pcg``, the same operations in the same
order. ``PcgConfig(neumann=("left", "right"))`` makes those sides Neumann
(``ConjugateGradient2D``'s rule: the ring there holds the outward difference, 0 for
an insulated wall); every level of the preconditioner then mirrors at them,
transfers included, and the iteration count stays where the all-Dirichlet one is
(docs/ARCHITECTURE.md "Neumann sides"). One process only.

Which solver when: ``MultigridPcg2D`` for a single-process Poisson or screened
solve of any size, with Dirichlet or Neumann sides; ``Multigrid2D`` where it applies (sides ``m 2^k - 1``, pure
Laplace weights) and a stand-alone cycle is wanted; ``ConjugateGradient2D`` for
very thin grids (it takes Neumann sides too); Chebyshev relaxation (``Stencil2D.run_until``) on decomposed
grids.

    python -m cuda_mpi_scratch_amd.models.pcg2d --size 2048x2048 --dtype f64 --source 4.77e-8 --boundary 0 --tol 1e-8
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from dataclasses import asdict, dataclass

import torch

from .._native import core, hip
from ..ops import cg, pcg
from ..parallel import DistContext
from .cg2d import _DTYPES, ConjugateGradient2D, _parse_wh


@dataclass
class PcgConfig:
    width: int = 2048
    height: int = 2048
    dtype: str = "f64"
    c_center: float = 0.2
    c_neighbor: float = 0.2
    nu_pre: int = 2
    nu_post: int = 2
    smoother_omega: float = 0.8
    coarse_reduction: float = 1e-3
    graph: bool = True
    check_every: int = 2
    neumann: tuple = ()  # the Neumann sides, any of "top", "bottom", "left", "right"; the others are Dirichlet

    def __post_init__(self):
        self.neumann = cg.neumann_sides(self.neumann)
        if self.dtype not in _DTYPES:
            raise ValueError(f"dtype must be f32 or f64, got {self.dtype!r}")
        if self.width < 1 or self.height < 1:
            raise ValueError("preconditioned CG: the grid must be non-empty")
        if self.check_every < 1:
            raise ValueError(f"preconditioned CG: check_every must be >= 1, got {self.check_every}")
        if self.nu_pre != self.nu_post:
            raise ValueError(f"preconditioned CG: nu_pre must equal nu_post (got {self.nu_pre}, {self.nu_post}): CG "
                             "needs a symmetric preconditioner")
        # The plan raises for inadmissible weights and for grids too thin to coarsen.
        core().pcg_plan_levels(int(self.width), int(self.height), float(self.c_center), float(self.c_neighbor),
                               list(self.neumann))
        core().mg_smoother_table(float(self.c_center), float(self.c_neighbor), float(self.smoother_omega),
                                 int(self.nu_pre))
        if not 0.0 < self.coarse_reduction < 1.0:
            raise ValueError("preconditioned CG: coarse_reduction must be in (0, 1)")


class MultigridPcg2D(ConjugateGradient2D):
    """``set_boundary / set_source / set_field / field / full / residual`` are
    ``ConjugateGradient2D``'s (the same tiles and the same native calls)."""

    def __init__(self, cfg: PcgConfig, ctx: DistContext | None = None, device: str | None = None):
        self.cfg = cfg
        self.ctx = ctx or DistContext()
        if self.ctx.world_size > 1:
            raise ValueError(f"MultigridPcg2D runs in one process (world size {self.ctx.world_size}): decomposed grids "
                             "are out of scope")
        self.device = torch.device(device) if device else self.ctx.device
        self.dtype = _DTYPES[cfg.dtype]
        self.iterations_run = 0
        self.levels = pcg.pcg_plan_levels(cfg.width, cfg.height, cfg.c_center, cfg.c_neighbor, cfg.neumann)
        if self.device.type == "cuda":
            with torch.cuda.device(self.device):
                self.solver = hip().PcgSolver(cfg.width, cfg.height, cfg.dtype, cfg.c_center, cfg.c_neighbor, cfg.nu_pre,
                                              cfg.smoother_omega, cfg.coarse_reduction, cfg.graph, list(cfg.neumann))
            self.geom = self.solver.geom()
        else:
            self.solver = None
            self.geom = core().TileGeom.compact(cfg.width, cfg.height, 1, 1)
            self._full = torch.zeros((cfg.height + 2, cfg.width + 2), dtype=self.dtype)
            self._g = torch.zeros((cfg.height, cfg.width), dtype=self.dtype)

    def solve(self, tol: float, max_iters: int = 1000, norm: str = "l2", check_every: int | None = None) -> dict:
        """Iterates from the current field until the residual's ``norm`` is ``<= tol``.
        The returned dict, the reasons and the restart rule are
        ``ConjugateGradient2D.solve``'s; ``check_every`` (how often the host looks,
        rounded up to even under a graph) changes no bit of the result."""
        if norm not in ("linf", "l2"):
            raise ValueError(f"solve: norm must be 'linf' or 'l2', got {norm!r}")
        if not tol >= 0 or max_iters < 0:
            raise ValueError(f"solve: needs tol >= 0 and max_iters >= 0, got {tol}, {max_iters}")
        every = self.cfg.check_every if check_every is None else int(check_every)
        if every < 1:
            raise ValueError(f"solve: check_every must be >= 1, got {every}")
        c = self.cfg
        if self.solver is not None:
            out = dict(self.solver.solve(float(tol), int(max_iters), norm, every))
            out["history"] = [tuple(h) for h in out["history"]]
        else:
            out = pcg.pcg_reference(self._full, self._g, c.c_center, c.c_neighbor, float(tol), int(max_iters), norm,
                                    c.nu_pre, c.smoother_omega, c.coarse_reduction, neumann=c.neumann)
            self._full = out.pop("full")
        self.iterations_run += out["iterations"]
        return out

    def scalars(self) -> dict:
        """The device scalar block (GPU only): ``rr, rz, pq, alpha, beta, linf, tol,
        iteration, max_iters, norm, status``."""
        if self.solver is None:
            raise RuntimeError("scalars(): the torch references keep no device block")
        return dict(self.solver.scalars())

    def note(self) -> str:
        if self.solver is not None:
            return self.solver.note()
        c, last = self.cfg, self.levels[-1]
        sides = f", Neumann sides {', '.join(c.neumann)}" if c.neumann else ""
        return (f"multigrid-preconditioned CG {c.width}x{c.height}, c_center {c.c_center:g}, c_neighbor "
                f"{c.c_neighbor:g}{sides}, V({c.nu_pre},{c.nu_post}) over {len(self.levels)} levels down to "
                f"{last['width']}x{last['height']}, torch references")


def main(argv=None) -> int:
    p = argparse.ArgumentParser(description="multigrid-preconditioned CG for the fixed-edge solve u = A u + g "
                                            "(MI355X-native)")
    p.add_argument("--size", default="2048x2048", help="core WxH, any sides that coarsen to at most 63")
    p.add_argument("--dtype", default="f64", choices=list(_DTYPES))
    p.add_argument("--source", type=float, default=None, metavar="Q", help="a constant source term g = Q")
    p.add_argument("--boundary", type=float, default=1.0, help="the top edge's value (the other edges hold 0)")
    p.add_argument("--tol", type=float, default=1e-8)
    p.add_argument("--max-iters", type=int, default=1000)
    p.add_argument("--norm", default="l2", choices=["linf", "l2"])
    p.add_argument("--c-center", type=float, default=0.2)
    p.add_argument("--c-neighbor", type=float, default=0.2)
    p.add_argument("--nu", type=int, default=2, help="pre- and post-smoothing sweeps (equal: a symmetric cycle)")
    p.add_argument("--smoother-omega", type=float, default=0.8)
    p.add_argument("--coarse-reduction", type=float, default=1e-3)
    p.add_argument("--check-every", type=int, default=2)
    p.add_argument("--neumann", default="", metavar="SIDES",
                   help="comma-separated Neumann (insulated) sides out of top,bottom,left,right; the others are Dirichlet")
    p.add_argument("--no-graph", action="store_true")
    p.add_argument("--device", default=None)
    p.add_argument("--json", default=None)
    args = p.parse_args(argv)
    w, h = _parse_wh(args.size)
    cfg = PcgConfig(width=w, height=h, dtype=args.dtype, c_center=args.c_center, c_neighbor=args.c_neighbor,
                    nu_pre=args.nu, nu_post=args.nu, smoother_omega=args.smoother_omega,
                    coarse_reduction=args.coarse_reduction, graph=not args.no_graph, check_every=args.check_every,
                    neumann=cg.neumann_sides(args.neumann))
    m = MultigridPcg2D(cfg, device=args.device)
    if "top" not in cfg.neumann:  # a Neumann top stays insulated
        m.set_boundary(top=args.boundary)
    m.set_source(args.source)
    if m.solver is not None:  # capture and warm up outside the timed region, then restore the start
        m.solve(args.tol, min(args.max_iters, 2 * args.check_every), args.norm)
        m.set_field(0.0)
        m.iterations_run = 0
    t0 = time.perf_counter()
    out = m.solve(args.tol, args.max_iters, args.norm)
    dt = time.perf_counter() - t0
    rec = {"metric": "pcg2d_solve_s", "value": dt, "config": asdict(cfg), "device": str(m.device), "note": m.note(),
           "graph": m.graph_status(), "source": args.source, "boundary": args.boundary,
           "neumann": list(cfg.neumann), "tol": args.tol,
           "norm": out["norm"], "converged": out["converged"], "iterations": out["iterations"],
           "residual": out["residual"], "reason": out["reason"], "restarts": out["restarts"],
           "levels": [(l["width"], l["height"]) for l in m.levels], "history": out["history"][-8:]}
    print(json.dumps(rec))
    if args.json:
        with open(args.json, "a") as f:
            f.write(json.dumps(rec) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
