"""Geometric multigrid V-cycles for the fixed-edge Poisson solve ``u = A u + g``.

``A u = c0 u + c1 (n + s + w + e)`` with ``c0 + 4 c1 = 1`` on a ``W x H`` core
whose depth-1 ring holds the Dirichlet values (docs/ARCHITECTURE.md
"Multigrid"). On a GPU ``Multigrid2D`` drives the native ``MultigridSolver`` (four
HIP kernels per level, one captured hipGraph per cycle); on the CPU it runs the
pure-torch references of ``ops.multigrid``, the same operations in the same
order. One process only: coarse levels of a decomposed grid would need
agglomeration.

    python -m cuda_mpi_scratch_amd.models.multigrid2d --size 2047x2047 --dtype f64 --source 1e-6 --tol 1e-8
"""
from __future__ import annotations

import argparse
import json
import math
import sys
import time
from dataclasses import asdict, dataclass

import torch

from .. import ops
from .._native import core, hip
from ..ops import multigrid as mg
from ..parallel import DistContext

_DTYPES = {"f32": torch.float32, "f64": torch.float64}
STALL_CYCLES = 3  # kMgStallCycles


@dataclass
class MultigridConfig:
    width: int = 2047
    height: int = 2047
    dtype: str = "f64"
    c_center: float = 0.2
    c_neighbor: float = 0.2
    nu_pre: int = 2
    nu_post: int = 2
    smoother_omega: float = 0.8
    coarse_reduction: float = 1e-3
    graph: bool = True

    def __post_init__(self):
        if self.dtype not in _DTYPES:
            raise ValueError(f"dtype must be f32 or f64, got {self.dtype!r}")
        if self.width < 1 or self.height < 1:
            raise ValueError("multigrid: the grid must be non-empty")
        core().mg_check_operator(float(self.c_center), float(self.c_neighbor))
        for name in ("nu_pre", "nu_post"):
            if not 1 <= getattr(self, name) <= core().MG_MAX_SMOOTH:
                raise ValueError(f"multigrid: {name} must be in 1..{core().MG_MAX_SMOOTH}, got {getattr(self, name)}")
        if not 0.0 < self.smoother_omega <= 1.0:
            raise ValueError("multigrid: smoother_omega must be in (0, 1]")
        if not 0.0 < self.coarse_reduction < 1.0:
            raise ValueError("multigrid: coarse_reduction must be in (0, 1)")


class Multigrid2D:
    def __init__(self, cfg: MultigridConfig, ctx: DistContext | None = None, device: str | None = None):
        self.cfg = cfg
        self.ctx = ctx or DistContext()
        if self.ctx.world_size > 1:
            raise ValueError(f"Multigrid2D runs in one process (world size {self.ctx.world_size}): decomposed grids "
                             "are out of scope, their coarse levels would need agglomeration")
        self.device = torch.device(device) if device else self.ctx.device
        self.dtype = _DTYPES[cfg.dtype]
        self._levels = mg.mg_plan_levels(cfg.width, cfg.height)  # raises for sizes that do not coarsen
        if len(self._levels) < 2:
            raise ValueError(f"multigrid: {cfg.width} x {cfg.height} has a single level (it coarsens only while both "
                             "sides are odd, >= 3 and the larger is above 31): nothing to cycle over")
        cw, ch = self._levels[-1]
        self._coarse = mg.mg_coarse_plan(cw, ch, cfg.c_center, cfg.c_neighbor, cfg.coarse_reduction)
        self.cycles_run = 0
        C = core()
        if self.device.type == "cuda":
            with torch.cuda.device(self.device):
                self.solver = hip().MultigridSolver(cfg.width, cfg.height, cfg.dtype, cfg.c_center, cfg.c_neighbor,
                                                    cfg.nu_pre, cfg.nu_post, cfg.smoother_omega, cfg.coarse_reduction,
                                                    cfg.graph)
            self.geom = self.solver.geom()
        else:
            self.solver = None
            self.geom = C.TileGeom.compact(cfg.width, cfg.height, 1, 1)
            self._full = torch.zeros((cfg.height + 2, cfg.width + 2), dtype=self.dtype)
            self._g = torch.zeros((cfg.height, cfg.width), dtype=self.dtype)

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
        as it is (the ring starts at 0)."""
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
        """``{"linf", "l2", "cells"}`` of ``r = (A u + g) - u`` over the core: the HIP
        kernel ``stencil5_residual`` with the source, or its CPU reference."""
        if self.solver is not None:
            r = self.solver.residual()
            return {"linf": float(r["linf"]), "l2": float(r["l2"]), "cells": int(r["cells"])}
        linf, l2 = ops.residual5_reference(self._full, 1, self.cfg.c_center, self.cfg.c_neighbor, source=self._g)
        return {"linf": linf, "l2": l2, "cells": self.cfg.width * self.cfg.height}

    def vcycle(self, n: int = 1):
        """``n`` V(nu_pre, nu_post) cycles."""
        if n < 0:
            raise ValueError("vcycle: n must be >= 0")
        c = self.cfg
        if self.solver is not None:
            self.solver.vcycle(int(n))
        elif n:
            self._full = mg.multigrid_vcycle_reference(self._full, self._g, c.c_center, c.c_neighbor, c.nu_pre, c.nu_post,
                                                       c.smoother_omega, c.coarse_reduction, cycles=n)
        self.cycles_run += n

    def solve(self, tol: float, max_cycles: int = 50, norm: str = "l2") -> dict:
        """Checks the residual first, then repeats ``vcycle(1)`` + ``residual()``.
        Returns ``{"converged", "cycles", "residual", "reason", "norm", "history":
        [(cycle, linf, l2), ...]}``; ``reason`` is ``"converged: <norm> residual <=
        tol"``, ``"max_cycles reached"``, ``"non-finite residual"`` or ``"stalled"``
        (no new best residual for 3 consecutive cycles: the element type's
        rounding floor)."""
        if norm not in ("linf", "l2"):
            raise ValueError(f"solve: norm must be 'linf' or 'l2', got {norm!r}")
        if not tol >= 0 or max_cycles < 0:
            raise ValueError(f"solve: needs tol >= 0 and max_cycles >= 0, got {tol}, {max_cycles}")
        if self.solver is not None:
            out = dict(self.solver.solve(float(tol), int(max_cycles), norm))
            out["history"] = [tuple(h) for h in out["history"]]
            self.cycles_run += out["cycles"]
            return out
        out = {"converged": False, "cycles": 0, "residual": 0.0, "reason": "", "norm": norm, "history": []}
        best, since_best = 0.0, 0
        while True:
            r = self.residual()
            out["residual"] = r[norm]
            out["history"].append((out["cycles"], r["linf"], r["l2"]))
            if not (math.isfinite(r[norm]) and math.isfinite(r["linf"])):
                out["reason"] = "non-finite residual"
                break
            if r[norm] <= tol:
                out["converged"] = True
                out["reason"] = f"converged: {norm} residual <= tol"
                break
            if out["cycles"] == 0 or r[norm] < best:
                best, since_best = r[norm], 0
            else:
                since_best += 1
                if since_best >= STALL_CYCLES:
                    out["reason"] = "stalled"
                    break
            if out["cycles"] >= max_cycles:
                out["reason"] = "max_cycles reached"
                break
            self.vcycle(1)
            out["cycles"] += 1
        return out

    # ------------------------------------------------------------------ notes
    def levels(self) -> list[tuple[int, int]]:
        """The levels, finest first, as ``(width, height)``."""
        return list(self._levels)

    def sweep_equivalents(self, cycles: int) -> float:
        """Fine-grid sweep equivalents of ``cycles`` cycles: ``(nu_pre + nu_post) 4 / 3`` each."""
        return cycles * (self.cfg.nu_pre + self.cfg.nu_post) * 4.0 / 3.0

    def graph_status(self) -> str:
        return self.solver.graph_status() if self.solver is not None else "off (torch references)"

    def note(self) -> str:
        if self.solver is not None:
            return self.solver.note()
        c, lv = self.cfg, self._levels
        return (f"multigrid V({c.nu_pre},{c.nu_post}), {len(lv)} levels {lv[0][0]}x{lv[0][1]} .. {lv[-1][0]}x{lv[-1][1]}, "
                f"smoother omega {c.smoother_omega:g}, coarse solve {self._coarse['repeats']} x {self._coarse['n']} "
                f"Chebyshev sweeps (rho {self._coarse['rho']:g}), torch references")


def _parse_wh(s: str) -> tuple[int, int]:
    w, h = s.lower().split("x")
    return int(w), int(h)


def main(argv=None) -> int:
    p = argparse.ArgumentParser(description="multigrid V-cycles for the fixed-edge Poisson solve (MI355X-native)")
    p.add_argument("--size", default="2047x2047", help="core WxH; sides m * 2^k - 1, m <= 64 (2047, 4095, 6143, 8191)")
    p.add_argument("--dtype", default="f64", choices=list(_DTYPES))
    p.add_argument("--source", type=float, default=None, metavar="Q", help="a constant source term g = Q")
    p.add_argument("--boundary", type=float, default=1.0, help="the top edge's value (the other edges hold 0)")
    p.add_argument("--tol", type=float, default=1e-8)
    p.add_argument("--max-cycles", type=int, default=50)
    p.add_argument("--norm", default="l2", choices=["linf", "l2"])
    p.add_argument("--nu-pre", type=int, default=2)
    p.add_argument("--nu-post", type=int, default=2)
    p.add_argument("--smoother-omega", type=float, default=0.8)
    p.add_argument("--coarse-reduction", type=float, default=1e-3)
    p.add_argument("--c-center", type=float, default=0.2)
    p.add_argument("--c-neighbor", type=float, default=0.2)
    p.add_argument("--no-graph", action="store_true")
    p.add_argument("--device", default=None)
    p.add_argument("--json", default=None)
    args = p.parse_args(argv)
    w, h = _parse_wh(args.size)
    cfg = MultigridConfig(width=w, height=h, dtype=args.dtype, c_center=args.c_center, c_neighbor=args.c_neighbor,
                          nu_pre=args.nu_pre, nu_post=args.nu_post, smoother_omega=args.smoother_omega,
                          coarse_reduction=args.coarse_reduction, graph=not args.no_graph)
    m = Multigrid2D(cfg, device=args.device)
    m.set_boundary(top=args.boundary)
    m.set_source(args.source)
    if m.solver is not None:  # capture and warm up outside the timed region, then restore the start
        m.vcycle(1)
        m.set_field(0.0)
        m.cycles_run = 0
    t0 = time.perf_counter()
    out = m.solve(args.tol, args.max_cycles, args.norm)
    dt = time.perf_counter() - t0
    rec = {"metric": "multigrid2d_solve_s", "value": dt, "config": asdict(cfg), "device": str(m.device),
           "levels": m.levels(), "note": m.note(), "graph": m.graph_status(), "source": args.source,
           "boundary": args.boundary, "tol": args.tol, "norm": out["norm"], "converged": out["converged"],
           "cycles": out["cycles"], "residual": out["residual"], "reason": out["reason"],
           "sweep_equivalents": m.sweep_equivalents(out["cycles"]), "history": out["history"]}
    print(json.dumps(rec))
    if args.json:
        with open(args.json, "a") as f:
            f.write(json.dumps(rec) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
