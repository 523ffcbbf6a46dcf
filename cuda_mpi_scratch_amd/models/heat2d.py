"""Implicit heat steps: the unconditionally stable theta-scheme for
``u_t = kappa lap(u) + f`` on one grid, each step one solve by ``MultigridPcg2D``
or ``ConjugateGradient2D``.

With ``lam = kappa dt / h^2`` (any ``lam > 0``: the explicit sweep of ``Stencil2D``
stops at 1/4), ``0.5 <= theta <= 1`` (1: backward Euler, 0.5: Crank-Nicolson) and
``D = 1 + 4 theta lam``, a step ``u -> u'`` is the fixed-edge problem ``u' = A u' +
g`` with ``c_center = 0``, ``c_neighbor = c1 = theta lam / D`` and ``g = a u + b (n + s
+ w + e) + q / D`` (``ops.heat``; docs/ARCHITECTURE.md "Implicit heat steps").
``set_source(q)`` takes ``q = dt f``. The sides are the solver's: Dirichlet values
in the ring, or on a Neumann side the outward difference (0: insulated); the
ring as it stands at the call is used at both time levels of a step, so for a
side that moves in time and Crank-Nicolson's second order supply the mean of
the two levels. On a GPU ``step`` is the native ``step()`` of the solver: one fused
HIP kernel makes the right-hand side and the first residual in a single pass
over ``u``, then the solver's own iterations run from ``u`` as the warm start. On
the CPU it runs ``ops.heat_step_reference``, the same operations in the same
order. One process only.

Accuracy: each step is solved to ``||r||_2 <= tol`` and ``lambda_min(L) >= 1 / D``, so
the error per step is at most ``D tol`` in l2: choose ``tol = eps / D`` for an error
``eps`` per step. fp32 amplifies the rounding of the right-hand side by up to ``D``
as well, so ``f64`` is recommended for stiff steps (large ``lam``), as the solvers
already say about their floors.

Which method: plain CG's iteration count grows like ``sqrt(1 + 8 theta lam)``
(the square root of the operator's condition number), that of the
multigrid-preconditioned CG does not. Measured on an MI355X at 2048 x 2048 in f64
(backward Euler, ``tol = 1e-10 ||u0||_2``): use ``"cg"`` below about ``lam = 4`` (1.4 ms
against 3.2 ms per step at ``lam = 0.25``, level at 4) and ``"pcg"`` above (4.3 ms against
14.7 ms at ``lam = 64``; docs/PERF.md "Implicit heat steps"). ``"cg"`` is also the one
for grids too thin to coarsen.

    python -m cuda_mpi_scratch_amd.models.heat2d --size 2048x2048 --lam 100 --theta 1 --steps 10 --tol 1e-10
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from dataclasses import asdict, dataclass

import torch

from ..ops import cg, heat
from ..parallel import DistContext
from .cg2d import _DTYPES, CgConfig, ConjugateGradient2D, _parse_wh
from .pcg2d import MultigridPcg2D, PcgConfig

METHODS = ("pcg", "cg")


@dataclass
class HeatConfig:
    width: int = 2048
    height: int = 2048
    dtype: str = "f64"
    lam: float = 1.0      # kappa dt / h^2 > 0
    theta: float = 1.0    # 1: backward Euler, 0.5: Crank-Nicolson
    method: str = "pcg"   # "pcg" (MultigridPcg2D) or "cg" (ConjugateGradient2D)
    neumann: tuple = ()   # the Neumann sides, any of "top", "bottom", "left", "right"; the others are Dirichlet
    graph: bool = True
    check_every: int | None = None  # None: the method's own default (pcg 2, cg 32)
    nu: int = 2
    smoother_omega: float = 0.8
    coarse_reduction: float = 1e-3

    def __post_init__(self):
        self.neumann = cg.neumann_sides(self.neumann)
        if self.method not in METHODS:
            raise ValueError(f"implicit heat step: method must be 'pcg' or 'cg', got {self.method!r}")
        heat.heat_coefficients(self.lam, self.theta)
        self.solver_config()

    def coefficients(self) -> dict:
        return heat.heat_coefficients(self.lam, self.theta)

    def solver_config(self):
        """The ``PcgConfig`` or ``CgConfig`` of the step's solve: weights ``(0, c1)``."""
        c1 = self.coefficients()["c1"]
        if self.method == "pcg":
            return PcgConfig(width=self.width, height=self.height, dtype=self.dtype, c_center=0.0, c_neighbor=c1,
                             nu_pre=self.nu, nu_post=self.nu, smoother_omega=self.smoother_omega,
                             coarse_reduction=self.coarse_reduction, graph=self.graph,
                             check_every=2 if self.check_every is None else self.check_every, neumann=self.neumann)
        return CgConfig(width=self.width, height=self.height, dtype=self.dtype, c_center=0.0, c_neighbor=c1,
                        graph=self.graph, check_every=32 if self.check_every is None else self.check_every,
                        neumann=self.neumann)


class ImplicitHeat2D:
    """``set_boundary / set_field / field / full / residual`` are the wrapped solver
    model's (``self.model``); after a step ``residual()`` is that step's true residual."""

    def __init__(self, cfg: HeatConfig, ctx: DistContext | None = None, device: str | None = None):
        self.cfg = cfg
        ctx = ctx or DistContext()
        if ctx.world_size > 1:
            raise ValueError(f"{type(self).__name__} runs in one process (world size {ctx.world_size}): decomposed "
                             "grids are out of scope")
        self.coeffs = cfg.coefficients()
        model = MultigridPcg2D if cfg.method == "pcg" else ConjugateGradient2D
        self.model = model(cfg.solver_config(), ctx, device)
        self.device, self.dtype, self.solver = self.model.device, self.model.dtype, self.model.solver
        self._q = None  # the CPU twin's source
        self.time_steps_total = 0
        self.unfinished = None  # the reason of a step that did not converge, until set_field

    # ------------------------------------------------------------------ set-up
    def set_boundary(self, top=None, bottom=None, left=None, right=None):
        """``ConjugateGradient2D.set_boundary``. It may be called between steps: the
        next step reads the ring as it then stands, at both of its time levels."""
        self.model.set_boundary(top, bottom, left, right)

    def set_field(self, u):
        self.model.set_field(u)
        self.unfinished = None

    def field(self) -> torch.Tensor:
        return self.model.field()

    def full(self) -> torch.Tensor:
        return self.model.full()

    def residual(self) -> dict:
        """The true residual of the last step's system (before the first step: of ``g = 0``)."""
        return self.model.residual()

    def set_source(self, q):
        """``q = dt f`` of the steps to come: a scalar, an ``(H, W)`` tensor or None (no
        source: the kernel then reads none). It is kept apart from the solver's
        ``g``, which every step overwrites with the step's right-hand side."""
        W, H = self.cfg.width, self.cfg.height
        if q is None:
            core_q = None
        elif isinstance(q, torch.Tensor):
            if q.dim() != 2 or tuple(q.shape) != (H, W):
                raise ValueError(f"set_source: q must be a scalar, None or a 2-D tensor of shape (H, W) = ({H}, {W}); "
                                 f"got {tuple(q.shape)}")
            core_q = q.to(device=self.device, dtype=self.dtype)
        else:
            core_q = torch.full((H, W), float(q), dtype=self.dtype, device=self.device)
        if self.solver is None:
            self._q = None if core_q is None else core_q.clone()
            return
        if core_q is None:
            self.solver.set_step_source(0)
            return
        tile = self.model._tile()
        self.model._core_of(tile).copy_(core_q)
        torch.cuda.synchronize(self.device)
        self.solver.set_step_source(tile.data_ptr())

    # ---------------------------------------------------------------- stepping
    def step(self, n: int = 1, tol: float = 1e-8, max_iters: int | None = None, norm: str = "l2",
             check_every: int | None = None) -> dict:
        """Takes up to ``n`` steps, each solved from the current field until the
        residual's ``norm`` is ``<= tol`` (at most ``max_iters`` iterations each; the
        method's default if None), and stops at the first that does not converge.
        Returns ``{"steps", "converged", "iterations": [...], "residuals": [...],
        "restarts": [...], "reason", "time_steps_total"}``: ``steps`` counts the
        converged ones, the lists have one entry per step tried. After a step that
        did not converge the field holds its unfinished iterate, not a time level:
        a further ``step`` raises until ``set_field`` gives a state to go on from."""
        if self.unfinished is not None:
            raise RuntimeError(f"step: the last step did not converge ({self.unfinished}), the field holds its unfinished "
                               "iterate; set_field a state to go on from")
        if n < 0:
            raise ValueError(f"step: n must be >= 0, got {n}")
        if norm not in ("linf", "l2"):
            raise ValueError(f"step: norm must be 'linf' or 'l2', got {norm!r}")
        cfg, m = self.cfg, self.model
        if max_iters is None:
            max_iters = 1000 if cfg.method == "pcg" else 10000
        if not tol >= 0 or max_iters < 0:
            raise ValueError(f"step: needs tol >= 0 and max_iters >= 0, got {tol}, {max_iters}")
        every = m.cfg.check_every if check_every is None else int(check_every)
        if every < 1:
            raise ValueError(f"step: check_every must be >= 1, got {every}")
        out = {"steps": 0, "converged": True, "iterations": [], "residuals": [], "restarts": [], "reason": ""}
        for _ in range(int(n)):
            if self.solver is not None:
                one = self.solver.step(float(cfg.lam), float(cfg.theta), float(tol), int(max_iters), norm, every)
            else:
                kw = ({"nu": cfg.nu, "smoother_omega": cfg.smoother_omega, "coarse_reduction": cfg.coarse_reduction}
                      if cfg.method == "pcg" else {})
                one = heat.heat_step_reference(m._full, self._q, cfg.lam, cfg.theta, float(tol), int(max_iters), norm,
                                               cfg.method, cfg.neumann, **kw)
                m._full, m._g = one["full"], one["g"]
            m.iterations_run += one["iterations"]
            out["iterations"].append(int(one["iterations"]))
            out["residuals"].append(float(one["residual"]))
            out["restarts"].append(int(one["restarts"]))
            out["reason"] = one["reason"]
            if not one["converged"]:
                out["converged"] = False
                self.unfinished = one["reason"]
                break
            out["steps"] += 1
            self.time_steps_total += 1
        out["time_steps_total"] = self.time_steps_total
        return out

    # ------------------------------------------------------------------ notes
    def graph_status(self) -> str:
        return self.model.graph_status()

    def note(self) -> str:
        c, h = self.cfg, self.coeffs
        scheme = "backward Euler" if c.theta == 1.0 else ("Crank-Nicolson" if c.theta == 0.5 else "theta-scheme")
        return (f"implicit heat step ({scheme}): lam {c.lam:g}, theta {c.theta:g}, D = 1 + 4 theta lam = {h['D']:g}, "
                f"c1 {h['c1']:.17g}, method {c.method}, error per step <= D tol in l2; {self.model.note()}")


def main(argv=None) -> int:
    p = argparse.ArgumentParser(description="implicit heat steps (backward Euler / Crank-Nicolson) on CG or "
                                            "multigrid-preconditioned CG (MI355X-native)")
    p.add_argument("--size", default="2048x2048", help="core WxH (pcg: any sides that coarsen to at most 63)")
    p.add_argument("--dtype", default="f64", choices=list(_DTYPES))
    p.add_argument("--lam", type=float, default=100.0, help="kappa dt / h^2 > 0")
    p.add_argument("--theta", type=float, default=1.0, help="1: backward Euler, 0.5: Crank-Nicolson")
    p.add_argument("--steps", type=int, default=10)
    p.add_argument("--tol", type=float, default=1e-10, help="the l2 (or linf) residual every step is solved to")
    p.add_argument("--max-iters", type=int, default=None, help="per step")
    p.add_argument("--norm", default="l2", choices=["linf", "l2"])
    p.add_argument("--method", default="pcg", choices=list(METHODS))
    p.add_argument("--neumann", default="", metavar="SIDES",
                   help="comma-separated Neumann (insulated) sides out of top,bottom,left,right; the others are Dirichlet")
    p.add_argument("--source", type=float, default=None, metavar="Q", help="a constant source q = dt f = Q")
    p.add_argument("--boundary", type=float, default=1.0, help="the top edge's value (the other edges hold 0)")
    p.add_argument("--check-every", type=int, default=None)
    p.add_argument("--no-graph", action="store_true")
    p.add_argument("--device", default=None)
    p.add_argument("--json", default=None)
    args = p.parse_args(argv)
    w, h = _parse_wh(args.size)
    cfg = HeatConfig(width=w, height=h, dtype=args.dtype, lam=args.lam, theta=args.theta, method=args.method,
                     neumann=cg.neumann_sides(args.neumann), graph=not args.no_graph, check_every=args.check_every)
    m = ImplicitHeat2D(cfg, device=args.device)
    if "top" not in cfg.neumann:  # a Neumann top stays insulated
        m.set_boundary(top=args.boundary)
    m.set_source(args.source)
    if m.solver is not None:  # capture and warm up outside the timed region, then restore the start
        m.step(1, args.tol, args.max_iters, args.norm)
        m.set_field(0.0)
        m.time_steps_total = 0
        m.model.iterations_run = 0
    t0 = time.perf_counter()
    out = m.step(args.steps, args.tol, args.max_iters, args.norm)
    dt = time.perf_counter() - t0
    tried = max(1, len(out["iterations"]))
    rec = {"metric": "heat2d_step_s", "value": dt / tried, "total_s": dt, "config": asdict(cfg), "device": str(m.device),
           "note": m.note(), "graph": m.graph_status(), "source": args.source, "boundary": args.boundary,
           "neumann": list(cfg.neumann), "tol": args.tol, "norm": args.norm, "steps": out["steps"],
           "converged": out["converged"], "iterations": out["iterations"], "residuals": out["residuals"],
           "restarts": out["restarts"], "reason": out["reason"], "time_steps_total": out["time_steps_total"]}
    print(json.dumps(rec))
    if args.json:
        with open(args.json, "a") as f:
            f.write(json.dumps(rec) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
