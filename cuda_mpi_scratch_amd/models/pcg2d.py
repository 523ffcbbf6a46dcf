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

import sys
from dataclasses import dataclass

from .._native import core, hip
from ..ops import cg, pcg
from ..parallel import DistContext
from .cg2d import _DTYPES, ConjugateGradient2D, run_main, solver_parser


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

    _why_one_process = "decomposed grids are out of scope"

    def __init__(self, cfg: PcgConfig, ctx: DistContext | None = None, device: str | None = None):
        super().__init__(cfg, ctx, device)
        self.levels = pcg.pcg_plan_levels(cfg.width, cfg.height, cfg.c_center, cfg.c_neighbor, cfg.neumann)

    def _native_solver(self):
        c = self.cfg
        return hip().PcgSolver(c.width, c.height, c.dtype, c.c_center, c.c_neighbor, c.nu_pre, c.smoother_omega,
                               c.coarse_reduction, c.graph, list(c.neumann))

    def _reference_solve(self, tol: float, max_iters: int, norm: str) -> dict:
        c = self.cfg
        return pcg.pcg_reference(self._full, self._g, c.c_center, c.c_neighbor, tol, max_iters, norm, c.nu_pre,
                                 c.smoother_omega, c.coarse_reduction, neumann=c.neumann)

    def solve(self, tol: float, max_iters: int = 1000, norm: str = "l2", check_every: int | None = None) -> dict:
        """Iterates from the current field until the residual's ``norm`` is ``<= tol``.
        The returned dict, the reasons and the restart rule are
        ``ConjugateGradient2D.solve``'s; ``check_every`` (how often the host looks,
        rounded up to even under a graph) changes no bit of the result."""
        return super().solve(tol, max_iters, norm, check_every)

    def scalars(self) -> dict:
        """The device scalar block (GPU only): ``rr, rz, pq, alpha, beta, linf, tol,
        iteration, max_iters, norm, status``."""
        return super().scalars()

    def note(self) -> str:
        if self.solver is not None:
            return self.solver.note()
        c, last = self.cfg, self.levels[-1]
        sides = f", Neumann sides {', '.join(c.neumann)}" if c.neumann else ""
        return (f"multigrid-preconditioned CG {c.width}x{c.height}, c_center {c.c_center:g}, c_neighbor "
                f"{c.c_neighbor:g}{sides}, V({c.nu_pre},{c.nu_post}) over {len(self.levels)} levels down to "
                f"{last['width']}x{last['height']}, torch references")


def main(argv=None) -> int:
    p = solver_parser("multigrid-preconditioned CG for the fixed-edge solve u = A u + g (MI355X-native)",
                      "core WxH, any sides that coarsen to at most 63", max_iters=1000, check_every=2)
    p.add_argument("--nu", type=int, default=2, help="pre- and post-smoothing sweeps (equal: a symmetric cycle)")
    p.add_argument("--smoother-omega", type=float, default=0.8)
    p.add_argument("--coarse-reduction", type=float, default=1e-3)
    return run_main(p, argv, "pcg2d_solve_s", MultigridPcg2D, PcgConfig,
                    extra=lambda a: {"nu_pre": a.nu, "nu_post": a.nu, "smoother_omega": a.smoother_omega,
                                     "coarse_reduction": a.coarse_reduction},
                    record_extra=lambda m: {"levels": [(l["width"], l["height"]) for l in m.levels]})


if __name__ == "__main__":
    sys.exit(main())
