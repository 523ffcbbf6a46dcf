"""Geometric multigrid for the fixed-edge Poisson solve ``u = A u + g``: the four
HIP kernels' wrappers and their pure-torch references (any device and dtype).

The method is fixed in ``csrc/include/mxs/kernels/multigrid.hpp`` and
docs/ARCHITECTURE.md "Multigrid"; the level planner and the sweep tables come
from there (``core().mg_plan_levels`` ...), so the references and the native
solver run the same doubles. The references work on plain 2-D arrays: ``full`` is
the core plus its depth-1 ring, ``(H + 2, W + 2)``; ``g`` and ``e`` are core
sized. Every expression is a rounding contract with
``csrc/kernels/multigrid_device.hpp``:

* sweep ``l``: ``x' = fma(nb_l, (n + s) + (w + e), ce_l c)``, then ``+ T(w_l) g``
  (the product rounded, then the sum), ring cells held: the rounding points of
  ``jacobi_source_per_step_reference(hold=15)``;
* residual: ``r = (fma(c1, (n + s) + (w + e), c0 v) + g) - v``;
* restriction with the factor 4 folded in:
  ``g_c = (r_c + 0.5 ((rn + rs) + (rw + re))) + 0.25 ((rnw + rne) + (rsw + rse))``;
* prolongation: bilinear with ``e = 0`` outside the coarse core, added to ``u``
  (``mg_prolong_add_reference``).
"""
from __future__ import annotations

import torch

from .._native import core, hip
from .relaxation import _fma
from .stencil import _stream, dtype_name


# ----------------------------------------------------------------- the tables
def mg_plan_levels(width: int, height: int) -> list[tuple[int, int]]:
    """The levels of a ``width x height`` core, finest first, as ``(width,
    height)``: both axes coarsen together, ``n_c = (n - 1) / 2``, while both
    sides are odd, >= 3 and the larger is above 31. Raises ValueError when the
    coarsest level is above 63 on a side."""
    return [tuple(l) for l in core().mg_plan_levels(int(width), int(height))]


def mg_smoother_table(c_center=0.2, c_neighbor=0.2, smoother_omega=0.8, sweeps=2) -> dict:
    """``{"n", "center", "neighbor", "weight"}`` of ``sweeps`` damped-Jacobi
    sweeps: ``w = omega / (1 - c0)``, ``center = 1 - w + w c0``, ``neighbor = w c1``."""
    return dict(core().mg_smoother_table(float(c_center), float(c_neighbor), float(smoother_omega), int(sweeps)))


def mg_coarse_plan(width: int, height: int, c_center=0.2, c_neighbor=0.2, coarse_reduction=1e-3) -> dict:
    """The coarsest level's solve: the 32-level Leja-ordered Chebyshev cycle as a
    sweep table plus ``"repeats"`` and ``"rho"``."""
    return dict(core().mg_coarse_plan(int(width), int(height), float(c_center), float(c_neighbor),
                                      float(coarse_reduction)))


def _table(center, neighbor, weight):
    center, neighbor, weight = ([float(v) for v in x] for x in (center, neighbor, weight))
    if not center or len(center) != len(neighbor) or len(center) != len(weight):
        raise ValueError("a sweep table needs as many center, neighbor and weight entries, at least one")
    return center, neighbor, weight


# ------------------------------------------------------------- the references
def _sweep(u: torch.Tensor, g: torch.Tensor, ce: float, nb: float, wt: float) -> torch.Tensor:
    dt = u.dtype
    c = u[1:-1, 1:-1]
    sums = (u[:-2, 1:-1] + u[2:, 1:-1]) + (u[1:-1, :-2] + u[1:-1, 2:])
    prod = torch.tensor(ce, dtype=dt) * c
    new = _fma(nb, sums.contiguous(), prod.contiguous())
    p = torch.tensor(wt, dtype=dt) * g
    out = u.clone()
    out[1:-1, 1:-1] = new + p
    return out


def mg_smooth_reference(full: torch.Tensor, g: torch.Tensor, center, neighbor, weight) -> torch.Tensor:
    """``len(center)`` sweeps on ``full`` (core + ring 1) with the core-sized
    source ``g``; the ring never changes. Returns the new ``full``."""
    center, neighbor, weight = _table(center, neighbor, weight)
    if full.dim() != 2 or tuple(g.shape) != (full.shape[0] - 2, full.shape[1] - 2):
        raise ValueError("mg_smooth_reference: full must be g plus a ring of depth 1")
    u = full
    g = g.to(dtype=full.dtype, device=full.device)
    for ce, nb, wt in zip(center, neighbor, weight):
        u = _sweep(u, g, ce, nb, wt)
    return u.clone() if u is full else u


def mg_residual_reference(full: torch.Tensor, g: torch.Tensor, c_center=0.2, c_neighbor=0.2) -> torch.Tensor:
    """The core-sized residual ``(fma(c1, (n + s) + (w + e), c0 v) + g) - v`` in the element type."""
    dt = full.dtype
    v = full[1:-1, 1:-1]
    sums = (full[:-2, 1:-1] + full[2:, 1:-1]) + (full[1:-1, :-2] + full[1:-1, 2:])
    prod = torch.tensor(c_center, dtype=dt) * v
    a = _fma(c_neighbor, sums.contiguous(), prod.contiguous())
    return (a + g.to(dtype=dt, device=full.device)) - v


def mg_restrict_reference(r: torch.Tensor) -> torch.Tensor:
    """``4 R r`` by full weighting: coarse ``[I][J]`` from the nine fine cells around
    ``[2 I + 1][2 J + 1]`` of an odd x odd ``r``."""
    H, W = r.shape
    if H % 2 != 1 or W % 2 != 1 or H < 3 or W < 3:
        raise ValueError(f"mg_restrict_reference: needs odd sides >= 3, got {W} x {H}")
    c = r[1:-1:2, 1:-1:2]
    n, s = r[0:-2:2, 1:-1:2], r[2::2, 1:-1:2]
    w, e = r[1:-1:2, 0:-2:2], r[1:-1:2, 2::2]
    nw, ne = r[0:-2:2, 0:-2:2], r[0:-2:2, 2::2]
    sw, se = r[2::2, 0:-2:2], r[2::2, 2::2]
    return (c + 0.5 * ((n + s) + (w + e))) + 0.25 * ((nw + ne) + (sw + se))


def mg_residual_restrict_reference(full: torch.Tensor, g: torch.Tensor, c_center=0.2, c_neighbor=0.2) -> torch.Tensor:
    """The coarse right-hand side ``g_c = 4 R ((A u + g) - u)``, coarse-core sized."""
    return mg_restrict_reference(mg_residual_reference(full, g, c_center, c_neighbor))


def mg_prolong_reference(e: torch.Tensor) -> torch.Tensor:
    """``P e`` on the ``(2 h + 1) x (2 w + 1)`` fine core, bilinear with ``e = 0``
    outside the coarse core. ``e[I][J]`` (row ``I``, column ``J``) sits on fine row
    ``2 I + 1``, column ``2 J + 1``; with ``z`` = ``e`` inside a ring of zeros:
    odd row / odd column ``e[I][J]``; even row ``0.5 (e[I-1][J] + e[I][J])``; even
    column ``0.5 (e[I][J-1] + e[I][J])``; even / even
    ``0.25 ((e[I-1][J-1] + e[I][J-1]) + (e[I-1][J] + e[I][J]))``."""
    h, w = e.shape
    z = torch.zeros((h + 2, w + 2), dtype=e.dtype, device=e.device)
    z[1:-1, 1:-1] = e
    p = torch.zeros((2 * h + 1, 2 * w + 1), dtype=e.dtype, device=e.device)
    p[1::2, 1::2] = e
    p[0::2, 1::2] = 0.5 * (z[:-1, 1:-1] + z[1:, 1:-1])
    p[1::2, 0::2] = 0.5 * (z[1:-1, :-1] + z[1:-1, 1:])
    p[0::2, 0::2] = 0.25 * ((z[:-1, :-1] + z[1:, :-1]) + (z[:-1, 1:] + z[1:, 1:]))
    return p


def mg_prolong_add_reference(u_core: torch.Tensor, e: torch.Tensor) -> torch.Tensor:
    """``u + P e`` over the fine core (one rounded add per cell)."""
    if tuple(u_core.shape) != (2 * e.shape[0] + 1, 2 * e.shape[1] + 1):
        raise ValueError("mg_prolong_add_reference: u must be (2 h + 1) x (2 w + 1) for an h x w e")
    return u_core + mg_prolong_reference(e.to(dtype=u_core.dtype, device=u_core.device))


def mg_coarse_solve_reference(g: torch.Tensor, center, neighbor, weight, repeats: int) -> torch.Tensor:
    """``repeats`` x ``len(center)`` sweeps from ``e = 0`` with a zero ring; returns the core of ``e``."""
    center, neighbor, weight = _table(center, neighbor, weight)
    h, w = g.shape
    u = torch.zeros((h + 2, w + 2), dtype=g.dtype, device=g.device)
    for _ in range(int(repeats)):
        for ce, nb, wt in zip(center, neighbor, weight):
            u = _sweep(u, g, ce, nb, wt)
    return u[1:-1, 1:-1].clone()


def multigrid_vcycle_reference(full: torch.Tensor, g: torch.Tensor, c_center=0.2, c_neighbor=0.2, nu_pre=2, nu_post=2,
                               smoother_omega=0.8, coarse_reduction=1e-3, cycles=1) -> torch.Tensor:
    """``cycles`` V(nu_pre, nu_post) cycles on ``full`` (core + ring 1) with the
    core-sized source ``g``, composed of the four references in the order of the
    native solver: pre-smooth, restrict the residual, ``e = 0``, recurse (the
    coarsest level runs the coarse solve), prolong and add, post-smooth."""
    core().mg_check_operator(float(c_center), float(c_neighbor))
    h, w = g.shape
    levels = mg_plan_levels(w, h)
    if len(levels) < 2:
        raise ValueError(f"multigrid: {w} x {h} has a single level: nothing to cycle over")
    pre = mg_smoother_table(c_center, c_neighbor, smoother_omega, nu_pre)
    post = mg_smoother_table(c_center, c_neighbor, smoother_omega, nu_post)
    cw, ch = levels[-1]
    coarse = mg_coarse_plan(cw, ch, c_center, c_neighbor, coarse_reduction)
    g = g.to(dtype=full.dtype, device=full.device)

    def level(k, u, gk):
        if k + 1 == len(levels):
            e = mg_coarse_solve_reference(gk, coarse["center"], coarse["neighbor"], coarse["weight"], coarse["repeats"])
            out = torch.zeros_like(u)
            out[1:-1, 1:-1] = e
            return out
        u = mg_smooth_reference(u, gk, pre["center"], pre["neighbor"], pre["weight"])
        gc = mg_residual_restrict_reference(u, gk, c_center, c_neighbor)
        e = level(k + 1, torch.zeros((gc.shape[0] + 2, gc.shape[1] + 2), dtype=u.dtype, device=u.device), gc)
        u = u.clone()
        u[1:-1, 1:-1] = mg_prolong_add_reference(u[1:-1, 1:-1], e[1:-1, 1:-1])
        return mg_smooth_reference(u, gk, post["center"], post["neighbor"], post["weight"])

    u = full
    for _ in range(int(cycles)):
        u = level(0, u, g)
    return u.clone() if u is full else u


# ------------------------------------------------------------ the HIP kernels
def _need_gpu(t, who):
    if not t.is_cuda:
        raise TypeError(f"{who} runs the HIP kernel: GPU tensors only (CPU: {who}_reference)")


def mg_smooth(u_in, u_out, src, geom, center, neighbor, weight, stream=None) -> None:
    """``len(center)`` (1..4) fused sweeps on flat tiles of geometry ``geom`` (ring
    >= 1): reads ``u_in`` (core and ring) and the core of ``src``, writes the core
    of ``u_out``."""
    _need_gpu(u_in, "mg_smooth")
    center, neighbor, weight = _table(center, neighbor, weight)
    hip().mg_smooth(u_in.data_ptr(), u_out.data_ptr(), src.data_ptr(), geom, center, neighbor, weight, dtype_name(u_in),
                    _stream(stream))


def mg_residual_restrict(u, src, geom, coarse_src, coarse_geom, c_center=0.2, c_neighbor=0.2, stream=None) -> None:
    """Core of ``coarse_src`` = ``4 R ((A u + src) - u)``, residual and full weighting fused."""
    _need_gpu(u, "mg_residual_restrict")
    hip().mg_residual_restrict(u.data_ptr(), src.data_ptr(), geom, coarse_src.data_ptr(), coarse_geom, float(c_center),
                               float(c_neighbor), dtype_name(u), _stream(stream))


def mg_prolong_add(e, coarse_geom, u, geom, stream=None) -> None:
    """Core of ``u`` += ``P e`` in place; only the core of ``e`` is read."""
    _need_gpu(u, "mg_prolong_add")
    hip().mg_prolong_add(e.data_ptr(), coarse_geom, u.data_ptr(), geom, dtype_name(u), _stream(stream))


def mg_coarse_solve(src, e, geom, center, neighbor, weight, repeats, stream=None) -> None:
    """``repeats`` x ``len(center)`` sweeps from 0 in one workgroup; writes the core of ``e``."""
    _need_gpu(src, "mg_coarse_solve")
    center, neighbor, weight = _table(center, neighbor, weight)
    hip().mg_coarse_solve(src.data_ptr(), e.data_ptr(), geom, center, neighbor, weight, int(repeats), dtype_name(src),
                          _stream(stream))
