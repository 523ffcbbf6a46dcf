"""Stencil update ops: HIP kernels on GPU tensors, exact references on CPU.

GPU tensors go to the hand-written gfx950 kernels in ``csrc/kernels/stencil.hip``
(no PyTorch fallback for a device tensor). CPU tensors use the reference
implementations below, which evaluate the same formula in the same order

    out = fma(c_neighbor, (n + s) + (w + e), c_center * c)

(the fused multiply-add is emulated in float64 for fp32 tiles: the product of
two fp32 values is exact in fp64, so only the final rounding differs in rare
double-rounding cases — tests compare with a 1-ulp tolerance). The bit-exact
forms of the one-step references live in ``ops/exact.py``.
"""
from __future__ import annotations

import torch

from .._native import hip

_DT = {torch.float32: "f32", torch.float64: "f64"}


def dtype_name(t: torch.Tensor) -> str:
    try:
        return _DT[t.dtype]
    except KeyError:
        raise TypeError(f"unsupported dtype {t.dtype}; use float32 or float64") from None


def _stream(stream):
    return (stream or torch.cuda.current_stream()).cuda_stream


def stencil5(src: torch.Tensor, dst: torch.Tensor, geom, row_begin: int = 0, row_end: int | None = None,
             c_center: float = 0.2, c_neighbor: float = 0.2, variant: str = "auto", stream=None) -> None:
    """5-point update of core rows [row_begin, row_end) over the full core width."""
    row_end = geom.height if row_end is None else row_end
    if src.is_cuda:
        hip().stencil5_rows(src.data_ptr(), dst.data_ptr(), geom, row_begin, row_end, c_center, c_neighbor,
                            dtype_name(src), _stream(stream), variant)
    else:
        stencil5_reference(src, dst, geom, 0, geom.width, row_begin, row_end, c_center, c_neighbor)


def stencil5_rect(src, dst, geom, x0, x1, y0, y1, c_center=0.2, c_neighbor=0.2, stream=None) -> None:
    if src.is_cuda:
        hip().stencil5_rect(src.data_ptr(), dst.data_ptr(), geom, x0, x1, y0, y1, c_center, c_neighbor,
                            dtype_name(src), _stream(stream))
    else:
        stencil5_reference(src, dst, geom, x0, x1, y0, y1, c_center, c_neighbor)


def stencil_box(src, dst, geom, x0, x1, y0, y1, weights, stream=None) -> None:
    """(2R+1)^2 box stencil with row-major weights (R = 1 or 2)."""
    k = int(round(len(weights) ** 0.5))
    r = (k - 1) // 2
    if src.is_cuda:
        hip().stencil_box(src.data_ptr(), dst.data_ptr(), geom, x0, x1, y0, y1, r, [float(w) for w in weights],
                          dtype_name(src), _stream(stream))
    else:
        box_reference(src, dst, geom, x0, x1, y0, y1, weights)


def _core_view(t, geom):
    v = t.view(geom.total_height(), geom.pitch)
    return v, geom.halo_y, geom.x_origin + geom.halo_x


def stencil5_reference(src, dst, geom, x0, x1, y0, y1, c_center=0.2, c_neighbor=0.2) -> None:
    v, oy, ox = _core_view(src, geom)
    o, _, _ = _core_view(dst, geom)
    ys, xs = slice(oy + y0, oy + y1), slice(ox + x0, ox + x1)
    c = v[ys, xs]
    n = v[oy + y0 - 1:oy + y1 - 1, xs]
    s = v[oy + y0 + 1:oy + y1 + 1, xs]
    w = v[ys, ox + x0 - 1:ox + x1 - 1]
    e = v[ys, ox + x0 + 1:ox + x1 + 1]
    sums = (n + s) + (w + e)
    if src.dtype == torch.float32:
        c1 = torch.tensor(c_neighbor, dtype=torch.float32).double()
        prod = (torch.tensor(c_center, dtype=torch.float32) * c).double()
        o[ys, xs] = (c1 * sums.double() + prod).float()
    else:
        o[ys, xs] = c_neighbor * sums + c_center * c


def box_reference(src, dst, geom, x0, x1, y0, y1, weights) -> None:
    k = int(round(len(weights) ** 0.5))
    r = (k - 1) // 2
    v, oy, ox = _core_view(src, geom)
    o, _, _ = _core_view(dst, geom)
    acc = torch.zeros((y1 - y0, x1 - x0), dtype=torch.float64)
    for ky in range(k):
        for kx in range(k):
            dy, dx = ky - r, kx - r
            wk = float(torch.tensor(float(weights[ky * k + kx]), dtype=torch.float32))  # kernel weights are fp32
            acc += wk * v[oy + y0 + dy:oy + y1 + dy, ox + x0 + dx:ox + x1 + dx].double()
    o[oy + y0:oy + y1, ox + x0:ox + x1] = acc.to(src.dtype)


def jacobi_reference_global(u: torch.Tensor, iters: int, c_center=0.2, c_neighbor=0.2,
                            periodic=True, boundary: float = 0.0) -> torch.Tensor:
    """Whole-grid reference for validating decompositions: a periodic torus, or
    (periodic=False) a grid whose outside ring holds the fixed value `boundary`
    (the models' physical edges: a ghost ring initialised once, never exchanged)."""
    u = u.clone()
    for _ in range(iters):
        if periodic:
            n, s = torch.roll(u, 1, 0), torch.roll(u, -1, 0)
            w, e = torch.roll(u, 1, 1), torch.roll(u, -1, 1)
        else:
            p = torch.nn.functional.pad(u[None, None], (1, 1, 1, 1), value=boundary)[0, 0]
            n, s = p[:-2, 1:-1], p[2:, 1:-1]
            w, e = p[1:-1, :-2], p[1:-1, 2:]
        sums = (n + s) + (w + e)
        if u.dtype == torch.float32:
            c1 = torch.tensor(c_neighbor, dtype=torch.float32).double()
            prod = (torch.tensor(c_center, dtype=torch.float32) * u).double()
            u = (c1 * sums.double() + prod).float()
        else:
            u = c_neighbor * sums + c_center * u
    return u


HOLD_TOP, HOLD_BOTTOM, HOLD_LEFT, HOLD_RIGHT = 1, 2, 4, 8  # kernels::HoldSide


def stencil5_tb_held(src, dst, geom, steps, x0, x1, y0, y1, c_center=0.2, c_neighbor=0.2, hold=15, stream=None) -> None:
    """``steps`` Jacobi iterations over core rectangle [x0, x1) x [y0, y1) of a
    ghost-ring tile beside fixed edges, in one launch (GPU tensors only): cells
    outside the core on a held side (``hold``: HOLD_* bits) keep their input
    value at every level, ghost cells on the other sides advance as cells.
    Per-step form: bitwise equal to ``steps`` single steps."""
    if not src.is_cuda:
        raise TypeError("stencil5_tb_held runs the HIP kernel: GPU tensors only (CPU: jacobi_held_reference)")
    hip().stencil5_tb_held(src.data_ptr(), dst.data_ptr(), geom, steps, x0, x1, y0, y1, c_center, c_neighbor,
                           int(hold), dtype_name(src), _stream(stream))


def jacobi_held_reference(full: torch.Tensor, steps: int, c_center=0.2, c_neighbor=0.2, hold: int = 15,
                          ring: int | None = None) -> torch.Tensor:
    """Reference of the time-blocked pass beside fixed edges on a full (core +
    ghost ring) 2-D array whose ring is ``ring`` cells deep (default: ``steps``).
    Every step updates all cells but the outermost ring of the array, then
    restores the cells outside the core on the held sides (``hold``: HOLD_*
    bits) to their input values. The stale outermost ring reaches one cell
    further in per step, so after ``steps <= ring`` steps the core is exact; the
    arithmetic is jacobi_reference_global's (fp32 through fp64)."""
    ring = steps if ring is None else ring
    if steps > ring:
        raise ValueError(f"jacobi_held_reference: {steps} steps need a ring of at least {steps} cells, got {ring}")
    u0 = full.clone()
    u = full.clone()
    H, W = u.shape
    for _ in range(steps):
        c = u[1:-1, 1:-1]
        sums = (u[:-2, 1:-1] + u[2:, 1:-1]) + (u[1:-1, :-2] + u[1:-1, 2:])
        if u.dtype == torch.float32:
            c1 = torch.tensor(c_neighbor, dtype=torch.float32).double()
            prod = (torch.tensor(c_center, dtype=torch.float32) * c).double()
            new = (c1 * sums.double() + prod).float()
        else:
            new = c_neighbor * sums + c_center * c
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


def jacobi_sum_reference_global(u: torch.Tensor, steps: int, c: float = 0.2) -> torch.Tensor:
    """One sum-form pass of `steps` levels on the periodic torus, in the exact
    association of the GPU sum bodies (stencil_bodies.hpp sum_rot4f / sum_w4d):
    v' = (n + s) + h3 with the horizontal 3-sum built from pair sums,
    h3(x) = (u[x] + u[x+1]) + u[x-1] for even x, (u[x-1] + u[x]) + u[x+1] for odd
    x, then one multiply by c^S — c first rounded to the element type as the
    per-step coefficient is, the power taken in fp64, then rounded — so the
    GPU's time-blocked sum-form pass must match it bit for bit (global x
    parity: the kernels' 4-cell lane vectors start at multiples of 4)."""
    v = u.clone()
    even = (torch.arange(u.shape[1]) % 2 == 0).to(u.device)
    for _ in range(steps):
        n, s = torch.roll(v, 1, 0), torch.roll(v, -1, 0)
        w, e = torch.roll(v, 1, 1), torch.roll(v, -1, 1)
        h3 = torch.where(even, (v + e) + w, (w + v) + e)
        v = (n + s) + h3
    c_t = float(torch.tensor(c, dtype=u.dtype))
    return v * torch.tensor(c_t ** steps, dtype=torch.float64).to(u.dtype)


def stencil5_residual(src: torch.Tensor, geom, c_center: float = 0.2, c_neighbor: float = 0.2, stream=None,
                      source: torch.Tensor | None = None):
    """``(linf, sumsq)`` of the Jacobi residual ``r = A u - u`` over the core of a
    ghost-ring tile: ``r = fma(c_neighbor, (n + s) + (w + e), c_center * v) - v``
    per cell in the element type, ``linf = max |r|`` (NaN if any is),
    ``sumsq = sum r^2`` in float64. GPU tensors run the HIP kernel
    (``csrc/kernels/residual.hip``: one streaming read of the core and the ring
    cells beside it, deterministic); CPU tensors the reference expression.
    ``source``: a tile of the same geometry whose core holds ``g`` of
    ``u' = A u + g``; then ``r = (fma(...) + g) - v``, each one rounded
    operation, and only core cells of ``source`` are read."""
    if geom.halo_x < 1 or geom.halo_y < 1:
        raise ValueError("stencil5_residual: the tile has no ghost ring (it needs one at least 1 deep)")
    if source is not None and (source.dtype != src.dtype or source.device != src.device
                               or source.numel() < geom.alloc_elems()):
        raise ValueError("stencil5_residual: source must be a tile of the field's geometry, dtype and device")
    if src.is_cuda:
        linf, sumsq = hip().stencil5_residual(src.data_ptr(), geom, c_center, c_neighbor, dtype_name(src),
                                              _stream(stream), source.data_ptr() if source is not None else 0)
        return float(linf), float(sumsq)
    cols = slice(geom.x_origin, geom.x_origin + geom.total_width())
    v = src.view(geom.total_height(), geom.pitch)[:, cols]
    g = None
    if source is not None:
        g = source.view(geom.total_height(), geom.pitch)[:, cols][geom.halo_y:geom.halo_y + geom.height,
                                                                  geom.halo_x:geom.halo_x + geom.width]
    r = _residual_field(v, (geom.halo_y, geom.halo_x), c_center, c_neighbor, g)
    return float(r.abs().max()) if r.numel() else 0.0, float((r * r).sum())


def _residual_field(full: torch.Tensor, ring, c_center, c_neighbor, source=None) -> torch.Tensor:
    """float64 residual of every core cell of a (total_height, total_width) view
    whose ring is ``ring`` = (rows, columns) deep: the stencil value rounded to
    the element type (jacobi_reference_global's arithmetic), plus the core-sized
    ``source`` if there is one (rounded), minus the cell, rounded to the element
    type again."""
    ry, rx = (ring, ring) if isinstance(ring, int) else ring
    if ry < 1 or rx < 1:
        raise ValueError("residual5_reference: the view has no ghost ring (it needs one at least 1 deep)")
    H, W = full.shape[0] - 2 * ry, full.shape[1] - 2 * rx
    c = full[ry:ry + H, rx:rx + W]
    n, s = full[ry - 1:ry - 1 + H, rx:rx + W], full[ry + 1:ry + 1 + H, rx:rx + W]
    w, e = full[ry:ry + H, rx - 1:rx - 1 + W], full[ry:ry + H, rx + 1:rx + 1 + W]
    sums = (n + s) + (w + e)
    if full.dtype == torch.float32:
        c1 = torch.tensor(c_neighbor, dtype=torch.float32).double()
        prod = (torch.tensor(c_center, dtype=torch.float32) * c).double()
        new = (c1 * sums.double() + prod).float()
    else:
        new = c_neighbor * sums + c_center * c
    if source is not None:
        new = new + source.to(dtype=full.dtype, device=full.device)
    return (new - c).double()


def residual5_reference(full: torch.Tensor, ring, c_center: float = 0.2, c_neighbor: float = 0.2, source=None):
    """CPU reference of the residual norms on a ``(total_height, total_width)``
    view (core + a ghost ring ``ring`` cells deep, an int or (rows, columns)):
    ``(linf, l2)`` of ``A u - u`` over the core, reduced in float64. Only the
    ring cells beside the core enter. ``source``: a core-sized 2-D tensor ``g``;
    then the norms are those of ``A u + g - u``."""
    r = _residual_field(full.detach().cpu(), ring, c_center, c_neighbor,
                        None if source is None else source.detach().cpu())
    if r.numel() == 0:
        return 0.0, 0.0
    return float(r.abs().max()), float(torch.sqrt((r * r).sum()))
