"""Multigrid-preconditioned conjugate gradients for the fixed-edge solve ``u = A u
+ g`` on any grid: the HIP kernels' wrappers and their pure-torch references (any
device and dtype).

The method is fixed in ``csrc/include/mxs/kernels/pcg.hpp`` and
docs/ARCHITECTURE.md "Preconditioned CG". CG on ``L u = b`` (``ops.cg``) is
preconditioned by ONE V-cycle from ``e = 0`` whose coarsening takes any side:
``n_c = floor(n / 2)``, coarse ``(I, J)`` on fine ``(2 I + 1, 2 J + 1)``. A coarse
level whose parent had an even height (width) REFLECTS its far rows (columns): the
ghost row ``H`` (column ``W``) reads as the negated last core row (column), a
Dirichlet zero half a coarse spacing away. The cycle is a fixed symmetric
positive-definite operator (``nu_pre == nu_post``); it need not converge alone.

The references work on plain 2-D arrays: ``full`` is the core plus a depth-1
ring, ``(H + 2, W + 2)``; ``g, r, z, p, q, e`` are core sized. Every expression is
a rounding contract with ``csrc/kernels/multigrid_device.hpp`` and ``cg.hip``, and each
is the one of ``ops.multigrid`` / ``ops.cg``; on a reflecting side the ghost is
``-c`` (exact) wherever a sweep or a residual reads it, the ring there is never
read. Sums (``rz = sum r z`` beside CG's) are float64 and differ from the
kernels' by the order of their terms only.

Neumann sides (``ops.cg``; docs/ARCHITECTURE.md "Neumann sides"): every level
carries four ghost codes ``top, bottom, left, right``: 0 the ring, -1 reflect, +1
MIRROR (the ghost is plus the neighbouring core cell). Level 0 has the solve's;
near sides of a coarse level inherit the kind; a far side is a mirror on every
level when the finest level's is, else the reflect rule above. The transfers see
the mirror too: the prolongation's coarse ghost equals the mirrored coarse cell,
and restriction, its exact transpose, counts the fine residual of a row / column
twice where the outer coarse neighbour is such a ghost. The references take the
codes as a trailing ``sides=(top, bottom, left, right)``; the flags stay and mean a
far code of -1.
"""
from __future__ import annotations

import math
import struct

import torch

from .._native import core, hip
from . import multigrid as mg
from .cg import (MAX_RESTARTS, NORMS, SIDES, _sums, _within, cg_apply_reference, cg_check_sides, cg_start_reference,
                 cg_update_reference, ghosted, neumann_sides, side_codes)
from .stencil import _stream, dtype_name, residual5_reference

_SCALARS = struct.Struct("<7d4i")  # kernels::PcgScalars
_FIELDS = ("rr", "rz", "pq", "alpha", "beta", "linf", "tol", "iteration", "max_iters", "norm", "status")
COARSEN_ABOVE = 31  # kMgCoarsenAbove
COARSEST_MAX = 63  # kMgCoarsestMax


# ------------------------------------------------------------------- the plan
def pcg_plan_levels(width: int, height: int, c_center=0.2, c_neighbor=0.2, neumann=()) -> list[dict]:
    """The preconditioner's levels, finest first: dicts ``width, height,
    reflect_rows, reflect_cols, c_center`` and the four ghost codes ``top, bottom,
    left, right`` (``core().pcg_plan_levels``). Raises ValueError naming
    ``ConjugateGradient2D`` when the coarsest level would be above 63 on a side, and
    for four Neumann sides on an unscreened operator."""
    return [dict(l) for l in core().pcg_plan_levels(int(width), int(height), float(c_center), float(c_neighbor),
                                                    list(neumann_sides(neumann)))]


def pcg_plan_levels_twin(width: int, height: int, c_center=0.2, c_neighbor=0.2, neumann=()) -> list[dict]:
    """``pcg_plan_levels`` in pure Python, operation for operation."""
    w, h, c0, c1 = int(width), int(height), float(c_center), float(c_neighbor)
    top, bottom, left, right = side_codes(neumann)
    if w < 1 or h < 1:
        raise ValueError("preconditioned CG: the grid must be non-empty")
    if not (c1 > 0.0) or not (c0 + 4.0 * c1 <= 1.0 + 1e-12) or not math.isfinite(c0):
        raise ValueError("preconditioned CG: needs c_neighbor > 0 and c_center + 4 c_neighbor <= 1")
    if top and bottom and left and right and abs(1.0 - c0 - 4.0 * c1) <= 1e-12:
        raise ValueError("neumann: with all four sides Neumann and c_center + 4 c_neighbor = 1 the operator is singular: "
                         "constants are its null space. Hold one side fixed (Dirichlet), or use a screened operator")
    sigma = 1.0 - c0 - 4.0 * c1
    if abs(sigma) <= 1e-12:
        sigma = 0.0
    lv = [{"width": w, "height": h, "reflect_rows": False, "reflect_cols": False, "c_center": c0,
           "top": top, "bottom": bottom, "left": left, "right": right}]
    scale = 1.0
    while max(w, h) > COARSEN_ABOVE and min(w, h) >= 2:
        scale *= 4.0
        rr, rc = not bottom and h % 2 == 0, not right and w % 2 == 0
        lv.append({"width": w // 2, "height": h // 2, "reflect_rows": rr, "reflect_cols": rc,
                   "c_center": c0 - (scale - 1.0) * sigma,
                   "top": top, "bottom": 1 if bottom else -int(rr), "left": left, "right": 1 if right else -int(rc)})
        w, h = w // 2, h // 2
    if w > COARSEST_MAX or h > COARSEST_MAX:
        raise ValueError(f"preconditioned CG: {width} x {height} is too thin to coarsen (it stops at {w} x {h}): "
                         "use ConjugateGradient2D")
    return lv


def level_sides(level: dict) -> tuple[int, int, int, int]:
    """The ghost codes ``(top, bottom, left, right)`` of a level dict; the four keys
    are optional (0, and -1 on a far side whose reflect flag is set)."""
    return _codes(level["reflect_rows"], level["reflect_cols"],
                  tuple(int(level.get(k, 0)) for k in SIDES))


def _codes(reflect_rows, reflect_cols, sides=None) -> tuple[int, int, int, int]:
    t, b, l, r = (0, 0, 0, 0) if sides is None else (int(v) for v in sides)
    if reflect_rows and b == 0:
        b = -1
    if reflect_cols and r == 0:
        r = -1
    if any(v not in (-1, 0, 1) for v in (t, b, l, r)):
        raise ValueError("ghost codes are 0 (ring), +1 (mirror) or -1 (reflect)")
    return t, b, l, r


def pcg_coarse_interval(level: dict, c_neighbor=0.2) -> tuple[float, float]:
    """``(a, b)`` of ``I - A`` the coarse solve of ``level`` is built on. With a mirror
    side ``a = 1 - c0 - c1 (mu_x + mu_y)`` is the smallest eigenvalue itself."""
    return tuple(core().pcg_coarse_interval(level["width"], level["height"], level["reflect_rows"],
                                            level["reflect_cols"], level["c_center"], float(c_neighbor),
                                            level_sides(level)))


def pcg_coarse_plan(level: dict, c_neighbor=0.2, coarse_reduction=1e-3) -> dict:
    """The coarsest level's solve as a sweep table plus ``"repeats"`` and ``"rho"``:
    ``mg_coarse_plan`` without a reflecting or mirror side, else the 32-point cycle
    on ``pcg_coarse_interval``."""
    return dict(core().pcg_coarse_plan(level["width"], level["height"], level["reflect_rows"], level["reflect_cols"],
                                       level["c_center"], float(c_neighbor), float(coarse_reduction),
                                       level_sides(level)))


def chebyshev_cycle_interval(a: float, b: float, c_center: float, c_neighbor: float, levels: int) -> dict:
    """``chebyshev_cycle`` on a given interval ``0 < a < b``."""
    return dict(core().chebyshev_cycle_interval(float(a), float(b), float(c_center), float(c_neighbor), int(levels)))


# ------------------------------------------------------------- the references
def _reflect(full: torch.Tensor, reflect_rows: bool, reflect_cols: bool, sides=None) -> torch.Tensor:
    """``full`` with the ghost row / column of every coded side set to minus
    (reflect) or plus (mirror) the neighbouring core row / column (a copy when
    anything changes)."""
    t, b, l, r = _codes(reflect_rows, reflect_cols, sides)
    if not (t or b or l or r):
        return full
    full = full.clone()
    if t:
        full[0, 1:-1] = -full[1, 1:-1] if t < 0 else full[1, 1:-1]
    if b:
        full[-1, 1:-1] = -full[-2, 1:-1] if b < 0 else full[-2, 1:-1]
    if l:
        full[1:-1, 0] = -full[1:-1, 1] if l < 0 else full[1:-1, 1]
    if r:
        full[1:-1, -1] = -full[1:-1, -2] if r < 0 else full[1:-1, -2]
    return full


def mgp_smooth_reference(full, g, center, neighbor, weight, reflect_rows=False, reflect_cols=False, *,
                         sides=None) -> torch.Tensor:
    """``mg_smooth_reference`` with coded ghosts: before every sweep the ghost of a
    reflecting (mirror) side is minus (plus) the current neighbouring core row /
    column. Returns the new ``full``; only its core is the kernel's output."""
    center, neighbor, weight = mg._table(center, neighbor, weight)
    if full.dim() != 2 or tuple(g.shape) != (full.shape[0] - 2, full.shape[1] - 2):
        raise ValueError("mgp_smooth_reference: full must be g plus a ring of depth 1")
    u = full.clone()
    g = g.to(dtype=full.dtype, device=full.device)
    for ce, nb, wt in zip(center, neighbor, weight):
        u = mg._sweep(_reflect(u, reflect_rows, reflect_cols, sides), g, ce, nb, wt)
    return u


def mgp_residual_restrict_reference(full, g, c_center=0.2, c_neighbor=0.2, reflect_rows=False,
                                    reflect_cols=False, *, sides=None) -> torch.Tensor:
    """``4 R r`` for a coarse core of ``(H // 2, W // 2)``: the residual reads the
    coded ghost, fine residuals outside the core count as 0. The transpose of the
    mirrored prolongation: a fine row / column whose outer coarse neighbour is a
    mirror ghost (row 0 under a mirror top, row ``H - 1`` under a mirror bottom when
    ``H`` is odd, the same for columns) counts twice, an exact doubling."""
    r = mg.mg_residual_reference(_reflect(full, reflect_rows, reflect_cols, sides), g, c_center, c_neighbor)
    H, W = r.shape
    if H < 2 or W < 2:
        raise ValueError("mgp_residual_restrict_reference: needs both sides >= 2")
    t, b, l, rt = _codes(reflect_rows, reflect_cols, sides)
    if t > 0 or b > 0 or l > 0 or rt > 0:
        r = r.clone()
        if t > 0:
            r[0, :] = r[0, :] + r[0, :]
        if b > 0 and H % 2 == 1:
            r[-1, :] = r[-1, :] + r[-1, :]
        if l > 0:
            r[:, 0] = r[:, 0] + r[:, 0]
        if rt > 0 and W % 2 == 1:
            r[:, -1] = r[:, -1] + r[:, -1]
    pad = torch.zeros((2 * (H // 2) + 1, 2 * (W // 2) + 1), dtype=r.dtype, device=r.device)
    pad[:H, :W] = r
    return mg.mg_restrict_reference(pad)


def mgp_prolong_add_reference(u_core: torch.Tensor, e: torch.Tensor, *, sides=None) -> torch.Tensor:
    """``u + P e`` over a fine core of any ``(H, W)`` with ``e`` of ``(H // 2, W // 2)``. On a
    mirror side the coarse ghost is the mirrored coarse cell (``e[-1] = e[0]``, ``e[CH] =
    e[CH - 1]``, the same for columns; a corner mirrors only where both its sides
    do); ring and reflect sides keep 0. ``mg_prolong_reference``'s expressions."""
    H, W = u_core.shape
    if tuple(e.shape) != (H // 2, W // 2) or H < 2 or W < 2:
        raise ValueError("mgp_prolong_add_reference: e must be (H // 2) x (W // 2)")
    e = e.to(dtype=u_core.dtype, device=u_core.device)
    t, b, l, r = _codes(False, False, sides)
    if not (t > 0 or b > 0 or l > 0 or r > 0):
        return u_core + mg.mg_prolong_reference(e)[:H, :W]
    h, w = e.shape
    z = torch.zeros((h + 2, w + 2), dtype=e.dtype, device=e.device)
    z[1:-1, 1:-1] = e
    if t > 0:
        z[0, :] = z[1, :]
    if b > 0:
        z[-1, :] = z[-2, :]
    if l > 0:
        z[:, 0] = z[:, 1]
    if r > 0:
        z[:, -1] = z[:, -2]
    p = torch.zeros((2 * h + 1, 2 * w + 1), dtype=e.dtype, device=e.device)
    p[1::2, 1::2] = e
    p[0::2, 1::2] = 0.5 * (z[:-1, 1:-1] + z[1:, 1:-1])
    p[1::2, 0::2] = 0.5 * (z[1:-1, :-1] + z[1:-1, 1:])
    p[0::2, 0::2] = 0.25 * ((z[:-1, :-1] + z[1:, :-1]) + (z[:-1, 1:] + z[1:, 1:]))
    return u_core + p[:H, :W]


def mgp_coarse_solve_reference(g, center, neighbor, weight, repeats, reflect_rows=False, reflect_cols=False, *,
                               sides=None):
    """``repeats`` x ``len(center)`` sweeps from ``e = 0`` with a zero ring and coded
    ghosts; returns the core of ``e``."""
    center, neighbor, weight = mg._table(center, neighbor, weight)
    h, w = g.shape
    u = torch.zeros((h + 2, w + 2), dtype=g.dtype, device=g.device)
    for _ in range(int(repeats)):
        for ce, nb, wt in zip(center, neighbor, weight):
            u = mg._sweep(_reflect(u, reflect_rows, reflect_cols, sides), g, ce, nb, wt)
    return u[1:-1, 1:-1].clone()


class PcgPlan:
    """Everything one preconditioner application needs, made once per grid and
    operator: the levels, a smoother table per level and the coarse solve."""

    def __init__(self, width, height, c_center=0.2, c_neighbor=0.2, nu=2, smoother_omega=0.8, coarse_reduction=1e-3,
                 neumann=()):
        self.c_neighbor = float(c_neighbor)
        self.neumann = neumann_sides(neumann)
        self.levels = pcg_plan_levels(width, height, c_center, c_neighbor, self.neumann)
        self.smooth = [mg.mg_smoother_table(l["c_center"], c_neighbor, smoother_omega, nu) for l in self.levels]
        self.coarse = pcg_coarse_plan(self.levels[-1], c_neighbor, coarse_reduction)


def pcg_precondition_reference(r: torch.Tensor, plan: PcgPlan) -> torch.Tensor:
    """``z = M r``: one V-cycle from 0 with ring 0 and source ``r``, composed of the
    references in the order of the native solver."""
    c1 = plan.c_neighbor

    def level(k, gk):
        l = plan.levels[k]
        rr, rc, sd = l["reflect_rows"], l["reflect_cols"], level_sides(l)
        if k + 1 == len(plan.levels):
            co = plan.coarse
            return mgp_coarse_solve_reference(gk, co["center"], co["neighbor"], co["weight"], co["repeats"], rr, rc,
                                              sides=sd)
        t = plan.smooth[k]
        u = torch.zeros((gk.shape[0] + 2, gk.shape[1] + 2), dtype=gk.dtype, device=gk.device)
        u = mgp_smooth_reference(u, gk, t["center"], t["neighbor"], t["weight"], rr, rc, sides=sd)
        gc = mgp_residual_restrict_reference(u, gk, l["c_center"], c1, rr, rc, sides=sd)
        e = level(k + 1, gc)
        v = torch.zeros_like(u)  # the ghosts are made anew from the core: start from the 0 ring
        v[1:-1, 1:-1] = mgp_prolong_add_reference(u[1:-1, 1:-1], e, sides=sd)
        u = mgp_smooth_reference(v, gk, t["center"], t["neighbor"], t["weight"], rr, rc, sides=sd)
        return u[1:-1, 1:-1].clone()

    return level(0, r.contiguous())


def pcg_reference(full: torch.Tensor, g: torch.Tensor, c_center=0.2, c_neighbor=0.2, tol=1e-8, max_iters=1000,
                  norm="l2", nu=2, smoother_omega=0.8, coarse_reduction=1e-3, *, neumann=()) -> dict:
    """The composed loop, step for step what the native solver runs: start, then
    per iteration ``z = M r``, ``rz' = sum r z``, ``beta = rz' / rz`` (0 on the
    first), apply with ``z``, ``alpha = rz / pq``, update. The host protocol and the
    returned dict are ``cg_reference``'s; ``neumann`` names the Neumann sides."""
    neumann = neumann_sides(neumann)
    cg_check_sides(c_center, c_neighbor, neumann)
    if norm not in NORMS:
        raise ValueError(f"pcg_reference: norm must be 'linf' or 'l2', got {norm!r}")
    if not tol >= 0 or max_iters < 0:
        raise ValueError("pcg_reference: needs tol >= 0 and max_iters >= 0")
    full = full.clone()
    g = g.to(dtype=full.dtype, device=full.device)
    plan = PcgPlan(g.shape[1], g.shape[0], c_center, c_neighbor, nu, smoother_omega, coarse_reduction, neumann)
    out = {"converged": False, "iterations": 0, "residual": 0.0, "reason": "", "norm": norm, "restarts": 0,
           "history": []}

    def true_residual():
        linf, l2 = residual5_reference(ghosted(full, neumann), 1, c_center, c_neighbor, source=g)
        return linf if norm == "linf" else l2, linf

    remaining, have_true = int(max_iters), False
    while True:
        r, rr, linf = cg_start_reference(full, g, c_center, c_neighbor, neumann=neumann)
        p, rz, it = torch.zeros_like(r), 0.0, 0
        out["history"].append((out["iterations"], linf, math.sqrt(rr)))
        status = 1 if _within(norm, rr, linf, tol) else (2 if remaining <= 0 else 0)
        while status == 0:
            z = pcg_precondition_reference(r, plan)
            rz_new = float((r.double() * z.double()).sum())
            beta = 0.0 if it == 0 else rz_new / rz
            rz = rz_new
            p, q, pq = cg_apply_reference(z, p, beta, c_center, c_neighbor, neumann=neumann)
            if not (pq > 0.0 and math.isfinite(pq)):
                status = 3
                break
            alpha = rz / pq
            u_new, r, rr, linf = cg_update_reference(full[1:-1, 1:-1], r, p, q, alpha)
            full[1:-1, 1:-1] = u_new
            it += 1
            out["history"].append((out["iterations"] + it, linf, math.sqrt(rr) if rr >= 0 else float("nan")))
            if _within(norm, rr, linf, tol):
                status = 1
            elif it >= remaining:
                status = 2
        out["iterations"] += it
        remaining -= it
        if status == 1:
            out["residual"], t_linf = true_residual()
            have_true = True
            if not (math.isfinite(out["residual"]) and math.isfinite(t_linf)):
                out["reason"] = "non-finite residual"
            elif out["residual"] <= tol:
                out["converged"] = True
                out["reason"] = f"converged: {norm} residual <= tol"
            elif out["restarts"] >= MAX_RESTARTS:
                out["reason"] = "stalled"
            elif remaining <= 0:
                out["reason"] = "max_iters reached"
            else:
                out["restarts"] += 1
                continue
        elif status == 2:
            out["reason"] = "max_iters reached"
        else:
            out["reason"] = "breakdown" if math.isfinite(rr) and math.isfinite(linf) else "non-finite residual"
        break
    if not have_true:
        out["residual"], _ = true_residual()
    out["full"] = full
    return out


# ------------------------------------------------------------ the HIP kernels
class PcgWorkspace:
    """What the launchers share on the device: the scalar block (``rr, rz, pq,
    alpha, beta, linf, tol`` as doubles, then ``iteration, max_iters, norm, status``
    as ints), the per-workgroup partials (enough for the ``pcg_*`` kernels and the
    smoother's dot epilogue) and the ticket (0 between launches)."""

    def __init__(self, geom, device):
        assert _SCALARS.size == hip().PCG_SCALARS_BYTES
        n = max(hip().cg_grid_size(geom), hip().mgp_smooth_grid_size(geom))
        self.scalars = torch.zeros(_SCALARS.size // 8, dtype=torch.float64, device=device)
        self.partials = torch.zeros(2 * n, dtype=torch.float64, device=device)
        self.counter = torch.zeros(1, dtype=torch.int32, device=device)

    def write(self, **values) -> None:
        """Sets the named members (``norm`` by name or number), keeps the others."""
        cur = self.read()
        cur.update(values)
        if isinstance(cur["norm"], str):
            cur["norm"] = NORMS[cur["norm"]]
        raw = bytearray(_SCALARS.pack(*(cur[k] for k in _FIELDS)))
        self.scalars.copy_(torch.frombuffer(raw, dtype=torch.float64))

    def read(self) -> dict:
        raw = self.scalars.cpu().numpy().tobytes()
        return dict(zip(_FIELDS, _SCALARS.unpack(raw)))

    def _ptrs(self):
        return self.scalars.data_ptr(), self.partials.data_ptr(), self.counter.data_ptr()


def _need_gpu(who, *tensors):
    for t in tensors:
        if not t.is_cuda:
            raise TypeError(f"{who} runs the HIP kernel: GPU tensors only (CPU: the references of ops.pcg)")
    if any(t.dtype != tensors[0].dtype for t in tensors):
        raise TypeError(f"{who}: the tiles must share one dtype")


def pcg_start(u, g, r, geom, c_center, c_neighbor, ws: PcgWorkspace, stream=None, *, neumann=()) -> None:
    """Core of ``r`` = ``(A u + g) - u``; ``ws`` gets ``rr, linf, rz = beta = 0, iteration =
    0`` and the status against its own ``tol, max_iters, norm``."""
    _need_gpu("pcg_start", u, g, r)
    hip().pcg_start(u.data_ptr(), g.data_ptr(), r.data_ptr(), geom, float(c_center), float(c_neighbor), *ws._ptrs(),
                    dtype_name(u), _stream(stream), side_codes(neumann))


def pcg_apply(z, p_old, p_new, q, geom, c_center, c_neighbor, ws: PcgWorkspace, stream=None, *, neumann=()) -> None:
    """Cores of ``p_new = fma(T(beta), p_old, z)`` and ``q = L p_new``; ``ws`` gets ``pq`` and
    ``alpha = rz / pq`` (or status 3). Stores nothing when ``ws`` holds a status != 0."""
    _need_gpu("pcg_apply", z, p_old, p_new, q)
    hip().pcg_apply(z.data_ptr(), p_old.data_ptr(), p_new.data_ptr(), q.data_ptr(), geom, float(c_center),
                    float(c_neighbor), *ws._ptrs(), dtype_name(z), _stream(stream), side_codes(neumann))


def pcg_update(u, r, p, q, geom, ws: PcgWorkspace, stream=None) -> None:
    """In place over the cores: ``u += alpha p``, ``r -= alpha q``; ``ws`` gets ``rr, linf``,
    the iteration count and the status (not ``beta``). Stores nothing when ``ws``
    holds a status != 0."""
    _need_gpu("pcg_update", u, r, p, q)
    hip().pcg_update(u.data_ptr(), r.data_ptr(), p.data_ptr(), q.data_ptr(), geom, *ws._ptrs(), dtype_name(u),
                     _stream(stream))


def mgp_smooth(u_in, u_out, src, geom, center, neighbor, weight, reflect_rows=False, reflect_cols=False,
               ws: PcgWorkspace | None = None, stream=None, *, sides=None) -> None:
    """``len(center)`` (1..4) fused sweeps with coded ghosts (``sides``: the four codes); writes the core of
    ``u_out``. With ``ws`` the launch also leaves ``rz = sum src u_out`` and ``beta``.
    ``u_in=None`` starts from a zero iterate without reading a tile for it."""
    if u_in is None:
        _need_gpu("mgp_smooth", u_out, src)
        center, neighbor, weight = mg._table(center, neighbor, weight)
        ptrs = ws._ptrs() if ws is not None else (0, 0, 0)
        hip().mgp_smooth(0, u_out.data_ptr(), src.data_ptr(), geom, center, neighbor, weight, bool(reflect_rows),
                         bool(reflect_cols), *ptrs, dtype_name(u_out), _stream(stream),
                         _codes(reflect_rows, reflect_cols, sides))
        return
    _need_gpu("mgp_smooth", u_in, u_out, src)
    center, neighbor, weight = mg._table(center, neighbor, weight)
    ptrs = ws._ptrs() if ws is not None else (0, 0, 0)
    hip().mgp_smooth(u_in.data_ptr(), u_out.data_ptr(), src.data_ptr(), geom, center, neighbor, weight,
                     bool(reflect_rows), bool(reflect_cols), *ptrs, dtype_name(u_in), _stream(stream),
                     _codes(reflect_rows, reflect_cols, sides))


def mgp_residual_restrict(u, src, geom, coarse_src, coarse_geom, c_center=0.2, c_neighbor=0.2, reflect_rows=False,
                          reflect_cols=False, stream=None, *, sides=None) -> None:
    """Core of ``coarse_src`` = ``4 R ((A u + src) - u)`` for a ``(W // 2) x (H // 2)`` coarse
    tile; the flags are the FINE level's."""
    _need_gpu("mgp_residual_restrict", u, src, coarse_src)
    hip().mgp_residual_restrict(u.data_ptr(), src.data_ptr(), geom, bool(reflect_rows), bool(reflect_cols),
                                coarse_src.data_ptr(), coarse_geom, float(c_center), float(c_neighbor), dtype_name(u),
                                _stream(stream), _codes(reflect_rows, reflect_cols, sides))


def mgp_prolong_add(e, coarse_geom, u, geom, stream=None, *, sides=None) -> None:
    """Core of ``u`` += ``P e`` in place for a ``(W // 2) x (H // 2)`` coarse tile; a mirror
    side of ``sides`` clamps the coarse index."""
    _need_gpu("mgp_prolong_add", e, u)
    hip().mgp_prolong_add(e.data_ptr(), coarse_geom, u.data_ptr(), geom, dtype_name(u), _stream(stream),
                          _codes(False, False, sides))


def mgp_coarse_solve(src, e, geom, center, neighbor, weight, repeats, reflect_rows=False, reflect_cols=False,
                     ws: PcgWorkspace | None = None, stream=None, *, sides=None) -> None:
    """``repeats`` x ``len(center)`` sweeps from 0 in one workgroup with coded ghosts;
    writes the core of ``e``. With ``ws`` it also leaves ``rz = sum src e`` and ``beta``."""
    _need_gpu("mgp_coarse_solve", src, e)
    center, neighbor, weight = mg._table(center, neighbor, weight)
    hip().mgp_coarse_solve(src.data_ptr(), e.data_ptr(), geom, center, neighbor, weight, int(repeats),
                           bool(reflect_rows), bool(reflect_cols), ws.scalars.data_ptr() if ws is not None else 0,
                           dtype_name(src), _stream(stream), _codes(reflect_rows, reflect_cols, sides))
