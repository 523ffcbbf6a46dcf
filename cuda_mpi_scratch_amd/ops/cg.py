"""Conjugate gradients for the fixed-edge solve ``u = A u + g``: the three HIP
kernels' wrappers and their pure-torch references (any device and dtype).

``A u = c0 u + c1 (n + s + w + e)`` on a ``W x H`` core whose depth-1 ring holds
the Dirichlet values. CG solves ``L u = b`` with ``L v = (1 - c0) v - c1 (n + s +
w + e)`` (``v = 0`` outside the core); the ring is folded into the right-hand
side, so the residual of the system is the project's own ``r = (A u + g) - u``.
The method is fixed in ``csrc/include/mxs/kernels/cg.hpp`` and
docs/ARCHITECTURE.md "Conjugate gradients". The references work on plain 2-D
arrays: ``full`` is the core plus its ring, ``(H + 2, W + 2)``; ``g, r, p, q`` are
core sized. Every expression is a rounding contract with ``csrc/kernels/cg.hip``:

* start: ``r = (fma(c1, (n + s) + (w + e), c0 v) + g) - v`` and ``p = r``
  (``mg_residual_reference``);
* apply: ``p' = fma(T(beta), p, r)``, ``q = fma(-c1, (n + s) + (w + e), T(1 - c0)
  p')`` with ``p' = 0`` outside the core;
* update: ``u = fma(T(alpha), p, u)``, ``r = fma(-T(alpha), q, r)``;
* every sum and scalar in float64: ``rr = sum r^2``, ``pq = sum p q``,
  ``alpha = rr / pq``, ``beta = rr' / rr``. The kernels' sums differ from the
  references' by the order of their terms only.

Neumann sides (``neumann=("left", "right")``, names as ``set_boundary`` has them;
docs/ARCHITECTURE.md "Neumann sides"): on such a side the ghost reads ``edge +
ring``, one addition in the element type, the ring cell holding the prescribed
outward difference ``d = u_ghost - u_edge`` (0: insulated). ``L`` stays symmetric
(its diagonal loses ``c1`` per Neumann side at an edge cell) and ``d`` is folded
into the right-hand side: apply reads the ghost as the edge cell of ``p'`` itself.
"""
from __future__ import annotations

import math
import struct

import torch

from .._native import core, hip
from .multigrid import mg_residual_reference
from .relaxation import fma
from .stencil import _stream, dtype_name, residual5_reference

NORMS = {"linf": 0, "l2": 1}  # kCgNormLinf, kCgNormL2
MAX_RESTARTS = 3  # kCgMaxRestarts
_SCALARS = struct.Struct("<6d4i")  # kernels::CgScalars
_FIELDS = ("rr", "pq", "alpha", "beta", "linf", "tol", "iteration", "max_iters", "norm", "status")


SIDES = ("top", "bottom", "left", "right")


def cg_check_operator(c_center: float, c_neighbor: float) -> None:
    """Raises ValueError unless ``c_neighbor > 0`` and ``c_center + 4 c_neighbor <= 1``."""
    core().cg_check_operator(float(c_center), float(c_neighbor))


def neumann_sides(neumann) -> tuple[str, ...]:
    """The Neumann sides as a tuple in the order top, bottom, left, right. Takes
    any collection of names (or one comma-separated string); unknown and repeated
    names raise ValueError."""
    if neumann is None:
        return ()
    names = [n.strip() for n in neumann.split(",") if n.strip()] if isinstance(neumann, str) else list(neumann)
    for n in names:
        if n not in SIDES:
            raise ValueError(f"neumann: unknown side {n!r} (the sides are top, bottom, left and right)")
        if names.count(n) > 1:
            raise ValueError(f"neumann: side {n!r} is named twice")
    return tuple(n for n in SIDES if n in names)


def side_codes(neumann) -> tuple[int, int, int, int]:
    """The ghost codes ``(top, bottom, left, right)`` of the solve: +1 on a Neumann
    side (mirror), 0 elsewhere (ring)."""
    names = neumann_sides(neumann)
    return tuple(int(n in names) for n in SIDES)


def cg_check_sides(c_center: float, c_neighbor: float, neumann=()) -> None:
    """``cg_check_operator``, and ValueError too when all four sides are Neumann with
    ``c_center + 4 c_neighbor = 1``: that operator is singular (constants are its null
    space); hold one side fixed or use a screened operator."""
    core().cg_check_sides(float(c_center), float(c_neighbor), list(neumann_sides(neumann)))


def ghosted(full: torch.Tensor, neumann=()) -> torch.Tensor:
    """``full`` as the operator reads it: the ghost of a Neumann side is ``edge + ring``
    (a copy when anything changes; corners are never read)."""
    names = neumann_sides(neumann)
    if not names:
        return full
    out = full.clone()
    if "top" in names:
        out[0, 1:-1] = full[1, 1:-1] + full[0, 1:-1]
    if "bottom" in names:
        out[-1, 1:-1] = full[-2, 1:-1] + full[-1, 1:-1]
    if "left" in names:
        out[1:-1, 0] = full[1:-1, 1] + full[1:-1, 0]
    if "right" in names:
        out[1:-1, -1] = full[1:-1, -2] + full[1:-1, -1]
    return out


# ------------------------------------------------------------- the references
def _sums(r: torch.Tensor) -> tuple[float, float]:
    d = r.double()
    return float((d * d).sum()), (float(d.abs().max()) if d.numel() else 0.0)


def _within(norm: str, rr: float, linf: float, tol: float) -> bool:
    return (linf if norm == "linf" else math.sqrt(rr)) <= tol


def cg_start_reference(full: torch.Tensor, g: torch.Tensor, c_center=0.2, c_neighbor=0.2, *, neumann=()):
    """``(r, rr, linf)``: the core-sized residual ``(A u + g) - u`` of ``full`` (core +
    ring 1), which is also the first direction, with ``sum r^2`` and ``max |r|``. On a
    Neumann side the ghost is ``edge + ring``."""
    r = mg_residual_reference(ghosted(full, neumann), g, c_center, c_neighbor).contiguous()
    return (r,) + _sums(r)


def cg_apply_reference(r: torch.Tensor, p_old: torch.Tensor, beta: float, c_center=0.2, c_neighbor=0.2, *,
                       neumann=()):
    """``(p_new, q, pq)``: the new direction ``fma(T(beta), p_old, r)``, ``q = L p_new``
    with ``p_new = 0`` outside the core (on a Neumann side: the edge cell of ``p_new``
    itself), and ``sum p_new q``."""
    dt = r.dtype
    p = fma(float(beta), p_old.contiguous(), r.contiguous())
    z = torch.zeros((p.shape[0] + 2, p.shape[1] + 2), dtype=dt, device=p.device)
    z[1:-1, 1:-1] = p
    names = neumann_sides(neumann)
    if "top" in names:
        z[0, 1:-1] = p[0]
    if "bottom" in names:
        z[-1, 1:-1] = p[-1]
    if "left" in names:
        z[1:-1, 0] = p[:, 0]
    if "right" in names:
        z[1:-1, -1] = p[:, -1]
    sums = (z[:-2, 1:-1] + z[2:, 1:-1]) + (z[1:-1, :-2] + z[1:-1, 2:])
    prod = torch.tensor(1.0 - float(c_center), dtype=dt) * p
    q = fma(-float(c_neighbor), sums.contiguous(), prod.contiguous())
    return p, q, float((p.double() * q.double()).sum())


def cg_update_reference(u: torch.Tensor, r: torch.Tensor, p: torch.Tensor, q: torch.Tensor, alpha: float):
    """``(u_new, r_new, rr, linf)`` over the core: ``u + alpha p`` and ``r - alpha q``,
    one fma each."""
    u_new = fma(float(alpha), p.contiguous(), u.contiguous())
    r_new = fma(-float(alpha), q.contiguous(), r.contiguous())
    return (u_new, r_new) + _sums(r_new)


def cg_reference(full: torch.Tensor, g: torch.Tensor, c_center=0.2, c_neighbor=0.2, tol=1e-8, max_iters=10000,
                 norm="l2", on_iteration=None, *, neumann=()) -> dict:
    """The composed loop, step for step what the native solver runs: start, then
    apply + update until the recursive residual's ``norm`` is ``<= tol``,
    ``max_iters`` iterations ran or ``pq`` is not positive and finite. A reported
    convergence is confirmed on the true residual; if that is above ``tol`` the
    loop starts again from the current field (at most 3 restarts, then
    ``"stalled"``). ``on_iteration(k, p, q)`` sees every direction. Returns
    ``{"full", "converged", "iterations", "residual", "reason", "norm", "restarts",
    "history": [(iteration, linf, l2), ...]}`` with one history entry per
    iteration and the true residual in ``"residual"``. ``neumann`` names the Neumann
    sides; the true residual is then that of the same operator."""
    neumann = neumann_sides(neumann)
    cg_check_sides(c_center, c_neighbor, neumann)
    if norm not in NORMS:
        raise ValueError(f"cg_reference: norm must be 'linf' or 'l2', got {norm!r}")
    if not tol >= 0 or max_iters < 0:
        raise ValueError("cg_reference: needs tol >= 0 and max_iters >= 0")
    full = full.clone()
    g = g.to(dtype=full.dtype, device=full.device)
    out = {"converged": False, "iterations": 0, "residual": 0.0, "reason": "", "norm": norm, "restarts": 0,
           "history": []}

    def true_residual():
        linf, l2 = residual5_reference(ghosted(full, neumann), 1, c_center, c_neighbor, source=g)
        return linf if norm == "linf" else l2, linf

    remaining, have_true = int(max_iters), False
    while True:
        r, rr, linf = cg_start_reference(full, g, c_center, c_neighbor, neumann=neumann)
        p, beta, it = r.clone(), 0.0, 0
        out["history"].append((out["iterations"], linf, math.sqrt(rr)))
        status = 1 if _within(norm, rr, linf, tol) else (2 if remaining <= 0 else 0)
        while status == 0:
            p, q, pq = cg_apply_reference(r, p, beta, c_center, c_neighbor, neumann=neumann)
            if not (pq > 0.0 and math.isfinite(pq)):
                status = 3
                break
            alpha = rr / pq
            if on_iteration is not None:
                on_iteration(out["iterations"] + it, p, q)
            u_new, r, rr_new, linf = cg_update_reference(full[1:-1, 1:-1], r, p, q, alpha)
            full[1:-1, 1:-1] = u_new
            beta, rr, it = rr_new / rr, rr_new, it + 1
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
class CgWorkspace:
    """What the three launchers share on the device: the scalar block (``rr, pq,
    alpha, beta, linf, tol`` as doubles, then ``iteration, max_iters, norm, status``
    as ints), the per-workgroup partials and the ticket (0 between launches)."""

    def __init__(self, geom, device):
        self.scalars = torch.zeros(_SCALARS.size // 8, dtype=torch.float64, device=device)
        self.partials = torch.zeros(2 * hip().cg_grid_size(geom), dtype=torch.float64, device=device)
        self.counter = torch.zeros(1, dtype=torch.int32, device=device)
        assert _SCALARS.size == hip().CG_SCALARS_BYTES

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
            raise TypeError(f"{who} runs the HIP kernel: GPU tensors only (CPU: {who}_reference)")
    if any(t.dtype != tensors[0].dtype for t in tensors):
        raise TypeError(f"{who}: the tiles must share one dtype")


def cg_start(u, g, r, p, geom, c_center, c_neighbor, ws: CgWorkspace, stream=None, *, neumann=()) -> None:
    """Cores of ``r`` and ``p`` = ``(A u + g) - u`` on flat tiles of geometry ``geom``
    (ring >= 1); ``ws`` gets ``rr, linf, beta = 0, iteration = 0`` and the status
    against its own ``tol, max_iters, norm``."""
    _need_gpu("cg_start", u, g, r, p)
    hip().cg_start(u.data_ptr(), g.data_ptr(), r.data_ptr(), p.data_ptr(), geom, float(c_center), float(c_neighbor),
                   *ws._ptrs(), dtype_name(u), _stream(stream), side_codes(neumann))


def cg_apply(r, p_old, p_new, q, geom, c_center, c_neighbor, ws: CgWorkspace, stream=None, *, neumann=()) -> None:
    """Cores of ``p_new = fma(T(beta), p_old, r)`` and ``q = L p_new``; ``ws`` gets ``pq``
    and ``alpha`` (or status 3). Stores nothing when ``ws`` holds a status != 0."""
    _need_gpu("cg_apply", r, p_old, p_new, q)
    hip().cg_apply(r.data_ptr(), p_old.data_ptr(), p_new.data_ptr(), q.data_ptr(), geom, float(c_center),
                   float(c_neighbor), *ws._ptrs(), dtype_name(r), _stream(stream), side_codes(neumann))


def cg_update(u, r, p, q, geom, ws: CgWorkspace, stream=None) -> None:
    """In place over the cores: ``u += alpha p``, ``r -= alpha q``; ``ws`` gets ``rr, linf,
    beta``, the iteration count and the status. Stores nothing when ``ws`` holds a
    status != 0."""
    _need_gpu("cg_update", u, r, p, q)
    hip().cg_update(u.data_ptr(), r.data_ptr(), p.data_ptr(), q.data_ptr(), geom, *ws._ptrs(), dtype_name(u),
                    _stream(stream))
