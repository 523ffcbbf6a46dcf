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
