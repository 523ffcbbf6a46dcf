"""Conjugate gradients for the fixed-edge solve ``u = A u + g`` on any grid.

``A u = c0 u + c1 (n + s + w + e)`` on a ``W x H`` core whose depth-1 ring holds
the Dirichlet values, any ``W, H >= 1`` and any weights with ``c1 > 0`` and
``c0 + 4 c1 <= 1``: the pure Laplace weights and every screened operator (the
backward-Euler heat step) below them (docs/ARCHITECTURE.md "Conjugate
gradients"). On a GPU ``ConjugateGradient2D`` drives the native ``CgSolver`` (two
HIP kernels per iteration with every dot product fused in, a captured hipGraph
per ``check_every`` iterations, the stopping test on the device); on the CPU it
runs the pure-torch references of ``ops.cg``, the same operations in the same
order. ``CgConfig(neumann=("left", "right"))`` makes those sides Neumann (insulated
walls, symmetry planes, prescribed fluxes): the ring there holds the outward
difference ``d = u_ghost - u_edge`` (``h du/dn``; 0 by default) instead of a value
(docs/ARCHITECTURE.md "Neumann sides"). One process only: a decomposed grid would need a halo exchange of the
direction and an all-reduce of the scalars.

Which solver when: ``Multigrid2D`` where it applies (sides ``m 2^k - 1``, pure
Laplace weights), it is far faster; ``ConjugateGradient2D`` for every other size
and for screened operators; Chebyshev relaxation (``Stencil2D.run_until``) on
decomposed grids.

    python -m cuda_mpi_scratch_amd.models.cg2d --size 2048x2048 --dtype f64 --source 4.77e-8 --boundary 0 --tol 1e-8
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from dataclasses import asdict, dataclass

import torch

from .. import ops
from .._native import core, hip
from ..ops import cg
from ..parallel import DistContext

_DTYPES = {"f32": torch.float32, "f64": torch.float64}


@dataclass
class CgConfig:
    width: int = 2048
    height: int = 2048
    dtype: str = "f64"
    c_center: float = 0.2
    c_neighbor: float = 0.2
    graph: bool = True
    check_every: int = 32
    neumann: tuple = ()  # the Neumann sides, any of "top", "bottom", "left", "right"; the others are Dirichlet

    def __post_init__(self):
        self.neumann = cg.neumann_sides(self.neumann)
        if self.dtype not in _DTYPES:
            raise ValueError(f"dtype must be f32 or f64, got {self.dtype!r}")
        if self.width < 1 or self.height < 1:
            raise ValueError("conjugate gradients: the grid must be non-empty")
        if self.check_every < 1:
            raise ValueError(f"conjugate gradients: check_every must be >= 1, got {self.check_every}")
        cg.cg_check_sides(self.c_center, self.c_neighbor, self.neumann)


class ConjugateGradient2D:
    # What a subclass on the same tiles and native calls (MultigridPcg2D) replaces.
    _why_one_process = ("decomposed grids are out of scope, they would need a halo exchange of the direction and an "
                        "all-reduce of the scalars")

    def __init__(self, cfg: CgConfig, ctx: DistContext | None = None, device: str | None = None):
        self.cfg = cfg
        self.ctx = ctx or DistContext()
        if self.ctx.world_size > 1:
            raise ValueError(f"{type(self).__name__} runs in one process (world size {self.ctx.world_size}): "
                             f"{self._why_one_process}")
        self.device = torch.device(device) if device else self.ctx.device
        self.dtype = _DTYPES[cfg.dtype]
        self.iterations_run = 0
        if self.device.type == "cuda":
            with torch.cuda.device(self.device):
                self.solver = self._native_solver()
            self.geom = self.solver.geom()
        else:
            self.solver = None
            self.geom = core().TileGeom.compact(cfg.width, cfg.height, 1, 1)
            self._full = torch.zeros((cfg.height + 2, cfg.width + 2), dtype=self.dtype)
            self._g = torch.zeros((cfg.height, cfg.width), dtype=self.dtype)

    def _native_solver(self):
        c = self.cfg
        return hip().CgSolver(c.width, c.height, c.dtype, c.c_center, c.c_neighbor, c.graph, list(c.neumann))

    def _reference_solve(self, tol: float, max_iters: int, norm: str) -> dict:
        c = self.cfg
        return cg.cg_reference(self._full, self._g, c.c_center, c.c_neighbor, tol, max_iters, norm, neumann=c.neumann)

    # ------------------------------------------------------------------ set-up
    def _core_of(self, tile: torch.Tensor) -> torch.Tensor:
        g = self.geom
        x0 = g.x_origin + g.halo_x
        return tile.view(g.total_height(), g.pitch)[g.halo_y:g.halo_y + g.height, x0:x0 + g.width]

    def _tile(self) -> torch.Tensor:
        return torch.zeros(self.geom.alloc_elems(), dtype=self.dtype, device=self.device)

    def set_boundary(self, top=None, bottom=None, left=None, right=None):
        """Dirichlet values of the ring: each argument is a scalar or a 1-D tensor
        over the width (top, bottom) or height (left, right); None leaves that side
        as it is (the ring starts at 0). On a Neumann side the values are the
        prescribed outward differences ``d = u_ghost - u_edge`` (0: insulated)."""
        def values(v, n, what):
            if v is None:
                return None
            if isinstance(v, torch.Tensor):
                if v.dim() != 1 or v.numel() != n:
                    raise ValueError(f"set_boundary: {what} must be a scalar or a 1-D tensor of {n} values")
                return v.to(device=self.device, dtype=self.dtype).contiguous()
            return torch.full((n,), float(v), device=self.device, dtype=self.dtype)

        W, H = self.cfg.width, self.cfg.height
        t, b = values(top, W, "top"), values(bottom, W, "bottom")
        l, r = values(left, H, "left"), values(right, H, "right")
        if self.solver is not None:
            torch.cuda.synchronize(self.device)
            self.solver.set_boundary(*(0 if v is None else v.data_ptr() for v in (t, b, l, r)))
            return
        f = self._full
        if t is not None:
            f[0, 1:-1] = t
        if b is not None:
            f[-1, 1:-1] = b
        if l is not None:
            f[1:-1, 0] = l
        if r is not None:
            f[1:-1, -1] = r

    def set_source(self, g):
        """The additive term ``g`` of ``u = A u + g``: a scalar, an ``(H, W)`` tensor
        or None (``g = 0``). For ``-laplace(u) = f`` with the 5-point average it is
        ``c_neighbor h^2 f``."""
        W, H = self.cfg.width, self.cfg.height
        if g is None:
            core_g = None
        elif isinstance(g, torch.Tensor):
            if g.dim() != 2 or tuple(g.shape) != (H, W):
                raise ValueError(f"set_source: g must be a scalar, None or a 2-D tensor of shape (H, W) = ({H}, {W}); "
                                 f"got {tuple(g.shape)}")
            core_g = g.to(device=self.device, dtype=self.dtype)
        else:
            core_g = torch.full((H, W), float(g), dtype=self.dtype, device=self.device)
        if self.solver is not None:
            if core_g is None:
                self.solver.set_source(0)
                return
            tile = self._tile()
            self._core_of(tile).copy_(core_g)
            torch.cuda.synchronize(self.device)
            self.solver.set_source(tile.data_ptr())
            return
        self._g = torch.zeros((H, W), dtype=self.dtype) if core_g is None else core_g.clone()

    def set_field(self, u):
        """The core of the field: a scalar or an ``(H, W)`` tensor. The ring stays."""
        W, H = self.cfg.width, self.cfg.height
        if isinstance(u, torch.Tensor):
            if tuple(u.shape) != (H, W):
                raise ValueError(f"set_field: u must be a scalar or a tensor of shape (H, W) = ({H}, {W})")
            core_u = u.to(device=self.device, dtype=self.dtype)
        else:
            core_u = torch.full((H, W), float(u), dtype=self.dtype, device=self.device)
        if self.solver is not None:
            tile = self._tile()
            self._core_of(tile).copy_(core_u)
            torch.cuda.synchronize(self.device)
            self.solver.set_field(tile.data_ptr())
            return
        self._full[1:-1, 1:-1] = core_u

    def full(self) -> torch.Tensor:
        """A copy of the field with its ring, ``(H + 2, W + 2)``."""
        if self.solver is None:
            return self._full.clone()
        tile = self._tile()
        torch.cuda.synchronize(self.device)
        self.solver.field(tile.data_ptr())
        g = self.geom
        return tile.view(g.total_height(), g.pitch)[:, g.x_origin:g.x_origin + g.total_width()].clone()

    def field(self) -> torch.Tensor:
        """A copy of the core of the field, ``(H, W)``."""
        return self.full()[1:-1, 1:-1].clone()

    # ---------------------------------------------------------------- solving
    def residual(self) -> dict:
        """``{"linf", "l2", "cells"}`` of the true residual ``r = (A u + g) - u`` over the
        core: the HIP kernel ``stencil5_residual`` with the source, or its CPU reference.
        With a Neumann side the ghost there is ``edge + ring`` on both devices (on the
        GPU the start kernel's residual; not to be called while a solve runs)."""
        if self.solver is not None:
            r = self.solver.residual()
            return {"linf": float(r["linf"]), "l2": float(r["l2"]), "cells": int(r["cells"])}
        linf, l2 = ops.residual5_reference(cg.ghosted(self._full, self.cfg.neumann), 1, self.cfg.c_center,
                                           self.cfg.c_neighbor, source=self._g)
        return {"linf": linf, "l2": l2, "cells": self.cfg.width * self.cfg.height}

    def solve(self, tol: float, max_iters: int = 10000, norm: str = "l2", check_every: int | None = None) -> dict:
        """Iterates from the current field until the residual's ``norm`` is ``<= tol``.
        Returns ``{"converged", "iterations", "residual", "reason", "norm", "restarts",
        "history": [(iteration, linf, l2), ...]}``: ``residual`` is the true one, the
        history that of the recursive residual at every check. ``reason`` is
        ``"converged: <norm> residual <= tol"``, ``"max_iters reached"``, ``"breakdown"``
        (``p . L p`` not positive), ``"non-finite residual"`` or ``"stalled"`` (the
        recursive residual met ``tol`` and the true one did not, after 3 restarts:
        the element type's floor). The device decides when the iteration stops, so
        ``check_every`` (how often the host looks) changes no bit of the result."""
        if norm not in ("linf", "l2"):
            raise ValueError(f"solve: norm must be 'linf' or 'l2', got {norm!r}")
        if not tol >= 0 or max_iters < 0:
            raise ValueError(f"solve: needs tol >= 0 and max_iters >= 0, got {tol}, {max_iters}")
        every = self.cfg.check_every if check_every is None else int(check_every)
        if every < 1:
            raise ValueError(f"solve: check_every must be >= 1, got {every}")
        if self.solver is not None:
            out = dict(self.solver.solve(float(tol), int(max_iters), norm, every))
            out["history"] = [tuple(h) for h in out["history"]]
        else:
            out = self._reference_solve(float(tol), int(max_iters), norm)
            self._full = out.pop("full")
        self.iterations_run += out["iterations"]
        return out

    # ------------------------------------------------------------------ notes
    def scalars(self) -> dict:
        """The device scalar block (GPU only): ``rr, pq, alpha, beta, linf, tol,
        iteration, max_iters, norm, status``."""
        if self.solver is None:
            raise RuntimeError("scalars(): the torch references keep no device block")
        return dict(self.solver.scalars())

    def graph_status(self) -> str:
        return self.solver.graph_status() if self.solver is not None else "off (torch references)"

    def note(self) -> str:
        if self.solver is not None:
            return self.solver.note()
        c = self.cfg
        sides = f", Neumann sides {', '.join(c.neumann)}" if c.neumann else ""
        return (f"conjugate gradients {c.width}x{c.height}, c_center {c.c_center:g}, c_neighbor {c.c_neighbor:g}{sides}, "
                "torch references")


def _parse_wh(s: str) -> tuple[int, int]:
    w, h = s.lower().split("x")
    return int(w), int(h)


def solver_parser(description: str, size_help: str, max_iters: int, check_every: int) -> argparse.ArgumentParser:
    """The flags cg2d and pcg2d share; a module adds its own before it calls ``run_main``."""
    p = argparse.ArgumentParser(description=description)
    p.add_argument("--size", default="2048x2048", help=size_help)
    p.add_argument("--dtype", default="f64", choices=list(_DTYPES))
    p.add_argument("--source", type=float, default=None, metavar="Q", help="a constant source term g = Q")
    p.add_argument("--boundary", type=float, default=1.0, help="the top edge's value (the other edges hold 0)")
    p.add_argument("--tol", type=float, default=1e-8)
    p.add_argument("--max-iters", type=int, default=max_iters)
    p.add_argument("--norm", default="l2", choices=["linf", "l2"])
    p.add_argument("--c-center", type=float, default=0.2)
    p.add_argument("--c-neighbor", type=float, default=0.2)
    p.add_argument("--check-every", type=int, default=check_every)
    p.add_argument("--neumann", default="", metavar="SIDES",
                   help="comma-separated Neumann (insulated) sides out of top,bottom,left,right; the others are Dirichlet")
    p.add_argument("--no-graph", action="store_true")
    p.add_argument("--device", default=None)
    p.add_argument("--json", default=None)
    return p


def run_main(p: argparse.ArgumentParser, argv, metric: str, model, config, extra=lambda args: {},
             record_extra=lambda m: {}) -> int:
    """Parse, build ``model(config(...))``, warm up, time one solve and emit the record.
    ``extra(args)``: the module's own config fields; ``record_extra(m)``: its own record keys."""
    args = p.parse_args(argv)
    w, h = _parse_wh(args.size)
    cfg = config(width=w, height=h, dtype=args.dtype, c_center=args.c_center, c_neighbor=args.c_neighbor,
                 graph=not args.no_graph, check_every=args.check_every, neumann=cg.neumann_sides(args.neumann),
                 **extra(args))
    m = model(cfg, device=args.device)
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
    rec = {"metric": metric, "value": dt, "config": asdict(cfg), "device": str(m.device), "note": m.note(),
           "graph": m.graph_status(), "source": args.source, "boundary": args.boundary,
           "neumann": list(cfg.neumann), "tol": args.tol,
           "norm": out["norm"], "converged": out["converged"], "iterations": out["iterations"],
           "residual": out["residual"], "reason": out["reason"], "restarts": out["restarts"],
           **record_extra(m), "history": out["history"][-8:]}
    print(json.dumps(rec))
    if args.json:
        with open(args.json, "a") as f:
            f.write(json.dumps(rec) + "\n")
    return 0


def main(argv=None) -> int:
    p = solver_parser("conjugate gradients for the fixed-edge solve u = A u + g (MI355X-native)",
                      "core WxH, any sides >= 1", max_iters=100000, check_every=32)
    return run_main(p, argv, "cg2d_solve_s", ConjugateGradient2D, CgConfig)


if __name__ == "__main__":
    sys.exit(main())
