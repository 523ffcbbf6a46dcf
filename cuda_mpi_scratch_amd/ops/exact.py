"""Bit-exact CPU references of the one-step kernels (``csrc/kernels/stencil_sweep.hpp``).

``stencil5_reference`` and ``box_reference`` (``ops/stencil.py``) stay within an
ulp or so of the kernels: the fp32 fused multiply-add goes through one float64
rounding and the fp64 one is not fused at all. The functions here evaluate the
kernels' documented chains with the correctly rounded ``fma`` of
``ops/relaxation.py`` in both types, so a one-step kernel must equal them bit
for bit (``tests/test_one_step_reference_cpu.py`` anchors them to exact rational
arithmetic):

* 5-point, ``jac()``: ``fma(c1, (n + s) + (w + e), c0 * c)``, every other
  operation one rounded operation of the element type, ``c0`` / ``c1`` rounded
  to the element type first;
* box: ``acc = 0``, then ``acc = fma(T(w_k), tap_k, acc)`` for ``ky`` outer,
  ``kx`` inner, the weights rounded to fp32 first.

The time-blocked pass (``csrc/kernels/stencil.hip``: ``stencil5_tb``) is held to
the same chain level by level: ``stencil5_exact_block_reference`` (per step, a
ghost ring as deep as the block) and ``jacobi_sum_block_reference`` (the sum
form's association on the same array).

They work on plain 2-D arrays (core + ghost ring, or the periodic core), not on
tiles.
"""
from __future__ import annotations

import torch

from .relaxation import fma


def _jac(c, n, s, w, e, c_center: float, c_neighbor: float) -> torch.Tensor:
    sums = (n + s) + (w + e)
    prod = torch.tensor(c_center, dtype=c.dtype) * c
    return fma(c_neighbor, sums.contiguous(), prod.contiguous())


def stencil5_exact_reference(full: torch.Tensor, c_center: float = 0.2, c_neighbor: float = 0.2) -> torch.Tensor:
    """One 5-point step on a ``(h + 2, w + 2)`` array (core + a ghost ring one
    cell deep): the ``(h, w)`` core, bitwise what ``jac()`` computes. The four
    ring corners are not read."""
    return _jac(full[1:-1, 1:-1], full[:-2, 1:-1], full[2:, 1:-1], full[1:-1, :-2], full[1:-1, 2:], c_center,
                c_neighbor)


def stencil5_exact_periodic_reference(u: torch.Tensor, steps: int = 1, c_center: float = 0.2,
                                      c_neighbor: float = 0.2) -> torch.Tensor:
    """``steps`` 5-point steps on the periodic ``(h, w)`` torus (``torch.roll``
    neighbours), each bitwise what ``jac()`` computes."""
    for _ in range(steps):
        u = _jac(u, torch.roll(u, 1, 0), torch.roll(u, -1, 0), torch.roll(u, 1, 1), torch.roll(u, -1, 1), c_center,
                 c_neighbor)
    return u


def stencil5_exact_block_reference(full: torch.Tensor, steps: int, c_center: float = 0.2,
                                   c_neighbor: float = 0.2) -> torch.Tensor:
    """The per-step time-blocked pass on a ghost-ring tile: ``steps``
    applications of ``stencil5_exact_reference`` to a ``(h + 2 steps, w + 2 steps)``
    array (core + a ghost ring ``steps`` deep). Every application drops the
    outermost ring, so what is left is the ``(h, w)`` core after ``steps`` steps,
    bitwise what ``stencil5_tb`` (``sum_form=False``, no wrap) must store."""
    if full.shape[0] <= 2 * steps or full.shape[1] <= 2 * steps:
        raise ValueError(f"stencil5_exact_block_reference: a {tuple(full.shape)} array has no core "
                         f"under a ring of {steps}")
    for _ in range(steps):
        full = stencil5_exact_reference(full, c_center, c_neighbor)
    return full


def jacobi_sum_block_reference(full: torch.Tensor, steps: int, c: float = 0.2) -> torch.Tensor:
    """The sum-form time-blocked pass on a ghost-ring tile: the ``(h, w)`` core of
    ``jacobi_sum_reference_global`` applied to the ``(h + 2 steps, w + 2 steps)``
    array as if it were a torus. A cell at least ``steps`` cells from the array's
    edge never sees the wrap, so the core is what the pass computes from the
    ring. The sum form pairs columns by the parity of the core column index
    (the kernels' 4-cell vectors start at core columns that are multiples of 4):
    with an odd ring the array gets one more column on the left, so that core
    column 0 lands on an even column of the torus."""
    if full.shape[0] <= 2 * steps or full.shape[1] <= 2 * steps:
        raise ValueError(f"jacobi_sum_block_reference: a {tuple(full.shape)} array has no core "
                         f"under a ring of {steps}")
    from .stencil import jacobi_sum_reference_global

    lead = steps % 2
    if lead:
        full = torch.nn.functional.pad(full, (1, 0))
    out = jacobi_sum_reference_global(full, steps, c)
    return out[steps:out.shape[0] - steps, steps + lead:out.shape[1] - steps].contiguous()


def box_exact_reference(full: torch.Tensor, weights) -> torch.Tensor:
    """The (2R+1)^2 box stencil with row-major ``weights`` on a ``(h + 2R, w + 2R)``
    array (core + a ghost ring R deep, corners included): the ``(h, w)`` core in
    the kernel's chain of fused multiply-adds."""
    k = int(round(len(weights) ** 0.5))
    r = (k - 1) // 2
    h, w = full.shape[0] - 2 * r, full.shape[1] - 2 * r
    acc = torch.zeros((h, w), dtype=full.dtype)
    for ky in range(k):
        for kx in range(k):
            wk = float(torch.tensor(float(weights[ky * k + kx]), dtype=torch.float32))  # kernel weights are fp32
            acc = fma(wk, full[ky:ky + h, kx:kx + w].contiguous(), acc)
    return acc
