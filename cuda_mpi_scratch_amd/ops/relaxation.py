"""Chebyshev relaxation cycles: the level table (a pure-Python twin of
``csrc/include/mxs/kernels/relaxation.hpp``), the level-table passes on the GPU
and their CPU reference.

A time-blocked pass of M levels becomes one M-point Chebyshev cycle: level
``l`` evaluates ``fma(neighbor[l], (n + s) + (w + e), center[l] * c)``, the
per-step expression with its own coefficient pair. The field is only meaningful
at cycle ends (inside a cycle it strays by up to ``growth`` x max|u|).
"""
from __future__ import annotations

import math

import torch

from .._native import hip
from .stencil import HOLD_BOTTOM, HOLD_LEFT, HOLD_RIGHT, HOLD_TOP, _stream, dtype_name

MAX_LEVELS = 32        # kernels::kMaxLevels
GROWTH_SAMPLES = 2048  # kernels::kGrowthSamples


def relaxation_spectrum(global_width: int, global_height: int, c_center: float, c_neighbor: float):
    """``(a, b)``: the interval that holds the spectrum of ``I - A`` on a grid
    with fixed edges on all four sides."""
    mu = (math.cos(math.pi / (global_width + 1)) + math.cos(math.pi / (global_height + 1))) / 2.0
    r = 4.0 * abs(c_neighbor) * mu
    return 1.0 - c_center - r, 1.0 - c_center + r


def chebyshev_cycle(global_width: int, global_height: int, c_center: float, c_neighbor: float, levels: int) -> dict:
    """The ``levels``-level Chebyshev cycle, operation for operation what
    ``kernels::chebyshev_cycle`` computes: ``{"n", "center", "neighbor",
    "growth", "omega", "roots"}`` with the levels in Leja order. Raises
    ValueError unless ``c_neighbor != 0`` and the lower end of the spectrum is
    positive (it is not for a periodic axis, nor for weights with
    ``c_center + 4 |c_neighbor| mu >= 1``)."""
    M = int(levels)
    if not 1 <= M <= MAX_LEVELS:
        raise ValueError(f"chebyshev_cycle: the cycle length must be in [1, {MAX_LEVELS}], got {M}")
    if global_width < 1 or global_height < 1:
        raise ValueError("chebyshev_cycle: the global grid must be non-empty")
    if not c_neighbor != 0.0:
        raise ValueError("chebyshev_cycle: c_neighbor must not be 0 (the relaxation needs the neighbours)")
    a, b = relaxation_spectrum(global_width, global_height, c_center, c_neighbor)
    if not a > 0.0:
        raise ValueError(f"chebyshev_cycle: the spectrum of I - A must be positive, but its lower end is {a:g} "
                         f"(c_center {c_center:g}, c_neighbor {c_neighbor:g} on {global_width} x {global_height}): "
                         "needs fixed edges on both axes and c_center + 4 |c_neighbor| mu < 1")
    mid, half = (a + b) / 2.0, (b - a) / 2.0
    root = [mid + half * math.cos(math.pi * float(2 * j + 1) / float(2 * M)) for j in range(M)]
    order, taken = [0], [False] * M
    taken[0] = True
    for l in range(1, M):
        best, best_p = -1, 0.0
        for k in range(M):
            if taken[k]:
                continue
            p = 1.0
            for q in range(l):
                p *= abs(root[k] - root[order[q]])
            if best < 0 or p > best_p * (1.0 + 1e-12):
                best, best_p = k, p
        order.append(best)
        taken[best] = True
    omega = [1.0 / root[j] for j in order]
    center = [1.0 - w + w * c_center for w in omega]
    neighbor = [w * c_neighbor for w in omega]
    growth = 0.0
    for k in range(GROWTH_SAMPLES + 1):
        x = mid + half * math.cos(math.pi * float(k) / float(GROWTH_SAMPLES))
        p = 1.0
        for w in omega:
            p *= 1.0 - w * x
            growth = max(growth, abs(p))
    return {"n": M, "center": center, "neighbor": neighbor, "growth": growth, "omega": omega,
            "roots": [root[j] for j in order]}


def _levels(center, neighbor):
    center, neighbor = [float(c) for c in center], [float(c) for c in neighbor]
    if len(center) != len(neighbor) or not center:
        raise ValueError("a level table needs as many center as neighbor coefficients, at least one")
    return center, neighbor


def _corr_ptr(corr, src, geom, who) -> int:
    if corr is None:
        return 0
    if corr.dtype != src.dtype or corr.device != src.device or corr.numel() < geom.alloc_elems():
        raise ValueError(f"{who}: corr must be a tile of the pass's geometry, dtype and device")
    return corr.data_ptr()


def stencil5_tb_levels(src, dst, geom, x0, x1, y0, y1, center, neighbor, stream=None, corr=None) -> None:
    """One pass of ``len(center)`` levels over core rectangle [x0, x1) x [y0, y1)
    of a ghost-ring tile at least that deep (GPU tensors only): level ``l`` is
    one Jacobi step with ``(center[l], neighbor[l])``. The contract of the
    per-step ``stencil5_tb`` without wrap, plus the table; bitwise equal to the
    single steps. Depths: fp32 20 / 24, fp64 12 / 16. ``corr``: a tile of the same
    geometry (a source term's correction); the pass then ends with
    ``dst += corr`` on the rectangle, one rounded add per cell, in the same
    launch, and reads only the rectangle's cells of ``corr``."""
    if not src.is_cuda:
        raise TypeError("stencil5_tb_levels runs the HIP kernels: GPU tensors only (CPU: jacobi_held_levels_reference)")
    center, neighbor = _levels(center, neighbor)
    hip().stencil5_tb_levels(src.data_ptr(), dst.data_ptr(), geom, x0, x1, y0, y1, center, neighbor, dtype_name(src),
                             _stream(stream), _corr_ptr(corr, src, geom, "stencil5_tb_levels"))


def stencil5_tb_held_levels(src, dst, geom, x0, x1, y0, y1, center, neighbor, hold=15, stream=None, corr=None) -> None:
    """``stencil5_tb_held`` with a level table: cells outside the core on a held
    side (``hold``: HOLD_* bits) keep their input value at every level; level
    ``l`` runs ``(center[l], neighbor[l])``. GPU tensors only; depths and ``corr``
    as for ``stencil5_tb_levels``."""
    if not src.is_cuda:
        raise TypeError("stencil5_tb_held_levels runs the HIP kernel: GPU tensors only "
                        "(CPU: jacobi_held_levels_reference)")
    center, neighbor = _levels(center, neighbor)
    hip().stencil5_tb_held_levels(src.data_ptr(), dst.data_ptr(), geom, x0, x1, y0, y1, center, neighbor, int(hold),
                                  dtype_name(src), _stream(stream), _corr_ptr(corr, src, geom, "stencil5_tb_held_levels"))


def _round_to_odd_sum(x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """x + y in float64 rounded to odd: the exact sum when it is representable,
    else the neighbour whose last mantissa bit is set. Rounding that to nearest
    in the same or a narrower format gives the correctly rounded x + y (Boldo &
    Melquiond, "Emulation of a FMA and correctly rounded sums", 2008)."""
    h = x + y
    z = h - x
    lo = (x - (h - z)) + (y - z)  # TwoSum: h + lo == x + y exactly
    bits = h.view(torch.int64)
    fix = (lo != 0) & ((bits & 1) == 0)
    away = (lo > 0) == (h > 0)  # the exact sum lies beyond h, away from zero
    step = torch.where(away, 1, -1).to(torch.int64)
    return torch.where(fix, (bits + step).view(torch.float64), h)


def _split(a: torch.Tensor):
    t = a * 134217729.0  # 2^27 + 1 (Veltkamp)
    hi = t - (t - a)
    return hi, a - hi


def fma(a, b: torch.Tensor, c: torch.Tensor) -> torch.Tensor:
    """fma(a, b, c) of the element type, correctly rounded. fp32 goes through
    float64, where a * b is exact; fp64 through error-free products and sums.
    (No overflow or subnormal handling: the fields this is used on are far from
    both.)"""
    if b.dtype == torch.float32:
        a64 = torch.tensor(a, dtype=torch.float32).double()
        return _round_to_odd_sum(a64 * b.double(), c.double()).float()
    a = torch.tensor(a, dtype=torch.float64)
    p = a * b
    ah, al = _split(a)
    bh, bl = _split(b)
    e = ((ah * bh - p) + ah * bl + al * bh) + al * bl  # TwoProduct: p + e == a * b exactly
    th = c + p
    z = th - c
    tl = (c - (th - z)) + (p - z)  # TwoSum: th + tl == c + p exactly
    return th + _round_to_odd_sum(tl, e)


_fma = fma  # the name it had while private


def jacobi_held_levels_reference(full: torch.Tensor, center_list, neighbor_list, hold: int = 15,
                                 ring: int | None = None) -> torch.Tensor:
    """``jacobi_held_reference`` with one coefficient pair per step: step ``l``
    evaluates ``fma(neighbor[l], (n + s) + (w + e), center[l] * c)`` on every
    cell but the outermost ring of the (core + ghost ring) array, then restores
    the cells outside the core on the held sides. Same formula and order as
    ``jacobi_held_reference``; the fused multiply-add is correctly rounded here
    (that function emulates it, within an ulp), because a cycle's level
    coefficients reach the hundreds and the level passes are compared bit for
    bit."""
    center, neighbor = _levels(center_list, neighbor_list)
    steps = len(center)
    ring = steps if ring is None else ring
    if steps > ring:
        raise ValueError(f"jacobi_held_levels_reference: {steps} steps need a ring of at least {steps} cells, got {ring}")
    u0 = full.clone()
    u = full.clone()
    H, W = u.shape
    dt = u.dtype
    for c0, c1 in zip(center, neighbor):
        c = u[1:-1, 1:-1]
        sums = (u[:-2, 1:-1] + u[2:, 1:-1]) + (u[1:-1, :-2] + u[1:-1, 2:])
        prod = torch.tensor(c0, dtype=dt) * c
        new = fma(c1, sums.contiguous(), prod.contiguous())
        u = u.clone()
        u[1:-1, 1:-1] = new
        if hold & HOLD_TOP:
            u[:ring, :] = u0[:ring, :]
        if hold & HOLD_BOTTOM:
            u[H - ring:, :] = u0[H - ring:, :]
        if hold & HOLD_LEFT:
            u[:, :ring] = u0[:, :ring]
        if hold & HOLD_RIGHT:
            u[:, W - ring:] = u0[:, W - ring:]
    return u
