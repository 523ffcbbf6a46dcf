"""Source term of a fixed-edge solve, ``u' = A u + g``: the references.

Level ``l`` of a cycle with a source is ``x' = C_l x + w_l g^`` (``C_l``: the
homogeneous level with the pair ``(center[l], neighbor[l])`` and the held ring
kept; ``w_l = neighbor[l] / c_neighbor``; ``g^`` = ``g`` on the core, 0 on the
ring). ``M`` levels compose to ``x_M = (C_{M-1} ... C_0) x_0 + G`` with
``G = sum_l (C_{M-1} ... C_{l+1}) w_l g^``, which depends on ``g`` and the table
only. So a cycle with a source is the homogeneous pass plus ``G`` added where
the pass stores (docs/ARCHITECTURE.md "Source term").

``source_correction_reference`` builds ``G`` by the recurrence the solvers run
(the same operations in the same order); ``jacobi_source_per_step_reference``
is the obvious definition, the source added at every level, in a torch dtype or
in ``numpy.longdouble``.
"""
from __future__ import annotations

import numpy as np
import torch

from .._native import core
from .relaxation import _fma, _levels
from .stencil import HOLD_BOTTOM, HOLD_LEFT, HOLD_RIGHT, HOLD_TOP, stencil5


def level_omega(neighbor_l: float, c_neighbor: float) -> float:
    """The weight of a level (``kernels::relaxation_omega``); 1 for a level that
    runs the base pair."""
    return 1.0 if neighbor_l == c_neighbor else neighbor_l / c_neighbor


def source_correction_reference(g_core: torch.Tensor, center, neighbor, c_neighbor: float,
                                dtype: torch.dtype | None = None) -> torch.Tensor:
    """The cycle's correction ``G`` over the core, on one rank: ``G_0 = 0``,
    ``G_{l+1} = C_l G_l + w_l g`` on a tile whose ring is 0. Each step is
    ``ops.stencil5`` (the HIP kernel for a GPU ``g_core``, the CPU reference
    otherwise), then ``p = T(w_l) * g`` rounded, then ``step + p`` rounded: what
    ``Stencil2D.set_source`` and ``StencilSolver::set_source`` compute, bit for
    bit. Returns a ``(height, width)`` tensor of ``dtype`` on ``g_core``'s device."""
    center, neighbor = _levels(center, neighbor)
    if g_core.dim() != 2:
        raise ValueError("source_correction_reference: g_core must be a 2-D tensor over the core")
    dtype = dtype or g_core.dtype
    h, w = g_core.shape
    dev = g_core.device
    g = g_core.to(dtype).contiguous()
    C = core()
    geom = C.TileGeom.aligned(w, h, 1, 1, g.element_size()) if dev.type == "cuda" else C.TileGeom.compact(w, h, 1, 1)
    a = torch.zeros(geom.alloc_elems(), dtype=dtype, device=dev)
    b = torch.zeros_like(a)

    def core_of(t):
        v = t.view(geom.total_height(), geom.pitch)
        x0 = geom.x_origin + geom.halo_x
        return v[geom.halo_y:geom.halo_y + h, x0:x0 + w]

    for c0, c1 in zip(center, neighbor):
        stencil5(a, b, geom, 0, h, c0, c1)
        p = torch.tensor(level_omega(c1, c_neighbor), dtype=dtype, device=dev) * g
        out = core_of(b)
        out.copy_(out + p)
        a, b = b, a
    if dev.type == "cuda":
        torch.cuda.synchronize(dev)
    return core_of(a).clone()


def jacobi_source_per_step_reference(full, g_core, center, neighbor, c_neighbor: float, hold: int = 15,
                                     cycles: int = 1, dtype=None):
    """The per-step iteration with the source at every level, ``cycles`` cycles
    of ``len(center)`` levels on a full (core + ring) 2-D array: every level
    updates all cells but the outermost ring of the array with
    ``fma(neighbor[l], (n + s) + (w + e), center[l] * c)``, adds
    ``w_l * g`` on the core and restores the cells outside the core on the held
    sides (``hold``: HOLD_* bits). The ring's depth is read from the shapes.

    ``dtype``: a torch dtype (default: ``full``'s) evaluates in that type with
    the kernels' rounding points (a correctly rounded fma, the product
    ``T(w_l) * g`` rounded, the sum rounded) and returns a tensor;
    ``numpy.longdouble`` evaluates the same expression in extended precision,
    with the coefficients first rounded to ``full``'s type (the values the
    kernels use), and returns a ``numpy.longdouble`` array."""
    center, neighbor = _levels(center, neighbor)
    ring = (full.shape[0] - g_core.shape[0]) // 2
    if ring < 1 or full.shape[0] - 2 * ring != g_core.shape[0] or full.shape[1] - 2 * ring != g_core.shape[1]:
        raise ValueError("jacobi_source_per_step_reference: full must be g_core plus a ring at least 1 deep")
    omega = [level_omega(n, c_neighbor) for n in neighbor]

    def restore(u, u0):
        H, W = u.shape
        if hold & HOLD_TOP:
            u[:ring, :] = u0[:ring, :]
        if hold & HOLD_BOTTOM:
            u[H - ring:, :] = u0[H - ring:, :]
        if hold & HOLD_LEFT:
            u[:, :ring] = u0[:, :ring]
        if hold & HOLD_RIGHT:
            u[:, W - ring:] = u0[:, W - ring:]

    if dtype is np.longdouble or dtype == np.longdouble:
        src_t = full.dtype if isinstance(full, torch.Tensor) else torch.float64
        rnd = lambda v: np.longdouble(float(torch.tensor(v, dtype=src_t).double()))  # noqa: E731
        u0 = (full.detach().cpu().double().numpy() if isinstance(full, torch.Tensor) else np.asarray(full)).astype(np.longdouble)
        g = (g_core.detach().cpu().double().numpy() if isinstance(g_core, torch.Tensor) else np.asarray(g_core)).astype(np.longdouble)
        u = u0.copy()
        for _ in range(cycles):
            for c0, c1, w in zip(center, neighbor, omega):
                sums = (u[:-2, 1:-1] + u[2:, 1:-1]) + (u[1:-1, :-2] + u[1:-1, 2:])
                new = rnd(c1) * sums + rnd(c0) * u[1:-1, 1:-1]
                u = u.copy()
                u[1:-1, 1:-1] = new
                u[ring:-ring, ring:-ring] += rnd(w) * g
                restore(u, u0)
        return u

    dt = dtype or full.dtype
    u0 = full.to(dt).clone()
    g = g_core.to(dtype=dt, device=u0.device)
    u = u0.clone()
    for _ in range(cycles):
        for c0, c1, w in zip(center, neighbor, omega):
            c = u[1:-1, 1:-1]
            sums = (u[:-2, 1:-1] + u[2:, 1:-1]) + (u[1:-1, :-2] + u[1:-1, 2:])
            prod = torch.tensor(c0, dtype=dt) * c
            new = _fma(c1, sums.contiguous(), prod.contiguous())
            u = u.clone()
            u[1:-1, 1:-1] = new
            p = torch.tensor(w, dtype=dt) * g
            u[ring:-ring, ring:-ring] = u[ring:-ring, ring:-ring] + p
            restore(u, u0)
    return u
