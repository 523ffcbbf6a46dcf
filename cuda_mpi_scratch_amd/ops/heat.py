"""Implicit heat steps: the theta-scheme for ``u_t = kappa lap(u) + f`` as the
project's own fixed-edge problem, its pure-torch references (any device and
dtype) and the wrappers of the fused HIP start kernels.

With ``lam = kappa dt / h^2 > 0``, ``0.5 <= theta <= 1`` (1: backward Euler, 0.5:
Crank-Nicolson) and ``D = 1 + 4 theta lam``, one step ``u -> u'`` solves
``u' = A u' + g`` with ``c_center = 0``, ``c_neighbor = c1 = theta lam / D`` and

    g = a u + b (n + s + w + e) + s q,
    a = (1 - 4 (1 - theta) lam) / D,  b = (1 - theta) lam / D,  s = 1 / D,  q = dt f

(``csrc/include/mxs/kernels/heat.hpp``; docs/ARCHITECTURE.md "Implicit heat
steps"). ``4 c1 = 1 - 1 / D < 1``: the operator is screened, legal with four
Neumann sides too, and ``lambda_min(L) >= 1 / D``, so a step solved to a residual
``r`` is off by at most ``D ||r||_2``. The ghosts of the explicit part are those
of ``cg_start``: the ring on a Dirichlet side, ``edge + ring`` on a Neumann side;
the ring as it stands is used at both time levels. The solve starts from ``u``.

Every expression is a rounding contract with ``cg_heat_start_kernel`` in
``csrc/kernels/cg.hip``; the coefficients are rounded to the element type once:

    S = (n + s) + (w + e)                 # a mirror ghost is c + ring, one addition
    g = fma(T(b), S, T(a) * c)            # always this expression, also when b == 0
    g = g + T(s) * q                      # only with a source: the product rounded, then the sum
    r = (fma(T(c1), S, T(0) * c) + g) - c # cg_start's expression on the rounded g
"""
from __future__ import annotations

import torch

from .._native import core, hip
from .cg import (CgWorkspace, _need_gpu, cg_reference, cg_start_reference, ghosted, neumann_sides, side_codes)
from .relaxation import fma
from .stencil import _stream, dtype_name


def heat_coefficients(lam: float, theta: float = 1.0) -> dict:
    """``{"lam", "theta", "D", "c1", "a", "b", "s"}`` of one theta-scheme step. Raises
    ValueError for ``lam <= 0``, non-finite input or ``theta`` outside ``[0.5, 1]``
    (below 0.5 the scheme is only conditionally stable: ``Stencil2D`` is the
    explicit stepper)."""
    lam, theta = float(lam), float(theta)
    h = dict(core().heat_coefficients(lam, theta))
    return {"lam": lam, "theta": theta, "D": 1.0 + 4.0 * theta * lam, **h}


def heat_rhs_reference(full: torch.Tensor, q, lam: float, theta: float = 1.0, neumann=()) -> torch.Tensor:
    """The core-sized right-hand side ``g`` of one step from ``full`` (core + ring 1)
    and the optional core-sized source ``q = dt f`` (None: no source), in the
    element type of ``full`` and in the kernel's order of operations."""
    h = heat_coefficients(lam, theta)
    dt = full.dtype
    gh = ghosted(full, neumann_sides(neumann))
    v = gh[1:-1, 1:-1]
    sums = (gh[:-2, 1:-1] + gh[2:, 1:-1]) + (gh[1:-1, :-2] + gh[1:-1, 2:])
    prod = torch.tensor(h["a"], dtype=dt) * v
    g = fma(h["b"], sums.contiguous(), prod.contiguous())
    if q is not None:
        g = g + torch.tensor(h["s"], dtype=dt) * q.to(dtype=dt, device=full.device)
    return g.contiguous()


def heat_start_reference(full: torch.Tensor, q, lam: float, theta: float = 1.0, neumann=()):
    """``(g, r, rr, linf)``: the step's right-hand side and the residual of the warm
    start, ``cg_start_reference`` of ``(full, g)`` with weights ``(0, c1)``: what the
    fused start kernel stores (``r`` is also plain CG's first direction)."""
    g = heat_rhs_reference(full, q, lam, theta, neumann)
    r, rr, linf = cg_start_reference(full, g, 0.0, heat_coefficients(lam, theta)["c1"], neumann=neumann)
    return g, r, rr, linf


def heat_step_reference(full: torch.Tensor, q, lam: float, theta: float = 1.0, tol=1e-8, max_iters=10000, norm="l2",
                        method="pcg", neumann=(), **pcg_kw) -> dict:
    """One step, step for step what the native ``step()`` runs: ``heat_rhs_reference``,
    then ``cg_reference`` (``method="cg"``) or ``pcg_reference`` (``"pcg"``; ``pcg_kw``:
    ``nu, smoother_omega, coarse_reduction``) from the current field. Returns that
    solve's dict (``"full"`` is the new field with the ring as it was) plus ``"g"``."""
    from .pcg import pcg_reference

    if method not in ("cg", "pcg"):
        raise ValueError(f"heat_step_reference: method must be 'cg' or 'pcg', got {method!r}")
    c1 = heat_coefficients(lam, theta)["c1"]
    g = heat_rhs_reference(full, q, lam, theta, neumann)
    if method == "cg":
        if pcg_kw:
            raise TypeError(f"heat_step_reference: method 'cg' takes no {sorted(pcg_kw)}")
        out = cg_reference(full, g, 0.0, c1, tol, max_iters, norm, neumann=neumann)
    else:
        out = pcg_reference(full, g, 0.0, c1, tol, max_iters, norm, neumann=neumann, **pcg_kw)
    out["g"] = g
    return out


# ------------------------------------------------------------ the HIP kernels
def _ptr(q):
    return 0 if q is None else q.data_ptr()


def cg_heat_start(u, q, g, r, p, geom, lam, theta, ws: CgWorkspace, stream=None, *, neumann=()) -> None:
    """The fused start of a step on flat tiles of geometry ``geom`` (ring >= 1): the
    cores of ``g`` (the right-hand side), ``r`` and ``p`` (the residual of the warm
    start) from ``u`` and the source tile ``q`` (None: the no-source kernel); ``ws``
    gets what ``cg_start`` gives it."""
    _need_gpu("cg_heat_start", *(t for t in (u, q, g, r, p) if t is not None))
    hip().cg_heat_start(u.data_ptr(), _ptr(q), g.data_ptr(), r.data_ptr(), p.data_ptr(), geom, float(lam), float(theta),
                        *ws._ptrs(), dtype_name(u), _stream(stream), side_codes(neumann))


def pcg_heat_start(u, q, g, r, geom, lam, theta, ws, stream=None, *, neumann=()) -> None:
    """``cg_heat_start`` on a ``PcgWorkspace``: the cores of ``g`` and ``r``, no first
    direction; ``ws`` gets what ``pcg_start`` gives it."""
    _need_gpu("pcg_heat_start", *(t for t in (u, q, g, r) if t is not None))
    hip().pcg_heat_start(u.data_ptr(), _ptr(q), g.data_ptr(), r.data_ptr(), geom, float(lam), float(theta), *ws._ptrs(),
                         dtype_name(u), _stream(stream), side_codes(neumann))
