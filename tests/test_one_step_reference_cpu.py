"""The bit-exact one-step references (ops/exact.py) against exact rational
arithmetic: every operation of the kernels' chains is evaluated on
``fractions.Fraction`` operands and rounded once, to the nearer of the two
neighbouring values of the element type (ties to even), never through a double.
This is what "bitwise" in tests/test_gpu_one_step.py rests on and, through the
level reference with unequal pairs, in tests/test_gpu_level_passes.py."""
import struct
from fractions import Fraction

import pytest
import torch

from cuda_mpi_scratch_amd import ops

DT = {"f32": torch.float32, "f64": torch.float64}
FMT = {"f32": ("<f", "<I", 23), "f64": ("<d", "<Q", 52)}
COEFFS = [(0.3, 0.15), (-37.25, 9.5)]
H, W = 6, 7


def _bits(x: float, dtype: str) -> int:
    f, i, _ = FMT[dtype]
    return struct.unpack(i, struct.pack(f, x))[0]


def _from_bits(b: int, dtype: str) -> float:
    f, i, _ = FMT[dtype]
    return struct.unpack(f, struct.pack(i, b))[0]


def _round(q: Fraction, dtype: str) -> float:
    """q rounded to nearest (ties to even) in the element type, decided in exact
    arithmetic among a first guess and its two neighbours. (Normal range only:
    the values here are far from overflow and from subnormals.)"""
    if q == 0:
        return 0.0
    sign = -1 if q < 0 else 1
    a = abs(q)
    guess = struct.unpack(FMT[dtype][0], struct.pack(FMT[dtype][0], float(a)))[0]  # near a, maybe not nearest
    b = _bits(guess, dtype)
    best = None
    for cand in (b - 1, b, b + 1):
        v = _from_bits(cand, dtype)
        err = abs(Fraction(v) - a)
        key = (err, cand & 1)  # nearer first, then the even mantissa
        if best is None or key < best[0]:
            best = (key, v)
    return sign * best[1]


def _cell(c, n, s, w, e, c0, c1, dtype):
    F = Fraction
    r = lambda q: F(_round(q, dtype))  # noqa: E731
    c0, c1 = r(F(c0)), r(F(c1))
    sums = r(r(F(n) + F(s)) + r(F(w) + F(e)))
    prod = r(c0 * F(c))
    return _round(c1 * sums + prod, dtype)  # the fma: one rounding of the exact c1 * sums + prod


def _field(shape, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(*shape, generator=g, dtype=torch.float64) * 2 - 1).to(DT[dtype])


def _differing(got: torch.Tensor, want_rows, dtype) -> int:
    want = torch.tensor(want_rows, dtype=torch.float64).to(DT[dtype])  # exact: every value is of the element type
    assert torch.equal(want.double(), torch.tensor(want_rows, dtype=torch.float64))
    return int((got != want).sum())


@pytest.mark.parametrize("c0,c1", COEFFS)
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_ghost_ring_reference_equals_rational_arithmetic(dtype, c0, c1):
    full = _field((H + 2, W + 2), dtype, 11)
    got = ops.stencil5_exact_reference(full, c0, c1)
    v = full.double().tolist()
    want = [[_cell(v[y][x], v[y - 1][x], v[y + 1][x], v[y][x - 1], v[y][x + 1], c0, c1, dtype)
             for x in range(1, W + 1)] for y in range(1, H + 1)]
    assert got.shape == (H, W) and got.dtype == DT[dtype]
    assert _differing(got, want, dtype) == 0


@pytest.mark.parametrize("c0,c1", COEFFS)
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_periodic_reference_equals_rational_arithmetic(dtype, c0, c1):
    u = _field((H, W), dtype, 12)
    v = u.double().tolist()
    for steps in (1, 2):
        v = [[_cell(v[y][x], v[(y - 1) % H][x], v[(y + 1) % H][x], v[y][(x - 1) % W], v[y][(x + 1) % W], c0, c1, dtype)
              for x in range(W)] for y in range(H)]
        assert _differing(ops.stencil5_exact_periodic_reference(u, steps, c0, c1), v, dtype) == 0


def _bit_view(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


@pytest.mark.parametrize("steps", [1, 2, 5, 9])
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_block_reference_equals_the_level_reference_on_the_core(dtype, steps):
    """S shrinking one-step applications against the level reference with no
    side held (which keeps the array's size and lets its stale outermost ring
    creep inwards): the same bits on the core, unequal coefficients."""
    c0, c1 = 0.5, 0.125
    full = _field((H + 2 * steps, W + 2 * steps), dtype, 20 + steps)
    got = ops.stencil5_exact_block_reference(full, steps, c0, c1)
    want = ops.jacobi_held_levels_reference(full, [c0] * steps, [c1] * steps, hold=0)[steps:-steps, steps:-steps]
    assert got.shape == (H, W) and got.dtype == DT[dtype]
    assert int((_bit_view(got) != _bit_view(want)).sum()) == 0
    # ... and against the torus: far enough from the edge the ring is the wrap.
    big = _field((H + 2 * steps + 3, W + 2 * steps + 2), dtype, 40 + steps)
    per = ops.stencil5_exact_periodic_reference(big, steps, c0, c1)[steps:-steps, steps:-steps]
    assert int((_bit_view(ops.stencil5_exact_block_reference(big, steps, c0, c1)) != _bit_view(per)).sum()) == 0


LEVELS = ([0.3, -1.75, 2.5], [0.15, 0.6875, -0.4])  # three unequal pairs: which level takes which is visible


def _held_levels_rational(full, center, neighbor, hold, ring, dtype):
    """The contract of ops.jacobi_held_levels_reference on lists and Fractions:
    level l updates every cell but the array's outermost ring with pair l, then
    the cells outside the core on a held side take their input values back."""
    u0 = full.double().tolist()
    rows, cols = len(u0), len(u0[0])
    u = [row[:] for row in u0]
    for c0, c1 in zip(center, neighbor):
        new = [row[:] for row in u]
        for y in range(1, rows - 1):
            for x in range(1, cols - 1):
                new[y][x] = _cell(u[y][x], u[y - 1][x], u[y + 1][x], u[y][x - 1], u[y][x + 1], c0, c1, dtype)
        for y in range(rows):
            for x in range(cols):
                if ((hold & ops.HOLD_TOP and y < ring) or (hold & ops.HOLD_BOTTOM and y >= rows - ring)
                        or (hold & ops.HOLD_LEFT and x < ring) or (hold & ops.HOLD_RIGHT and x >= cols - ring)):
                    new[y][x] = u0[y][x]
        u = new
    return u


@pytest.mark.parametrize("hold", [0, 15])
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_level_reference_equals_rational_arithmetic_with_unequal_levels(dtype, hold):
    """A 7 x 9 core with a ring of 3 and 3 levels of unequal pairs: the whole
    array, ring included, bit for bit; and the table is taken in its order (the
    reversed table gives another core)."""
    ring = 3
    center, neighbor = LEVELS
    full = _field((7 + 2 * ring, 9 + 2 * ring), dtype, 31)
    got = ops.jacobi_held_levels_reference(full, center, neighbor, hold=hold)
    assert got.shape == full.shape and got.dtype == DT[dtype]
    assert _differing(got, _held_levels_rational(full, center, neighbor, hold, ring, dtype), dtype) == 0
    back = ops.jacobi_held_levels_reference(full, center[::-1], neighbor[::-1], hold=hold)
    assert _differing(back, _held_levels_rational(full, center[::-1], neighbor[::-1], hold, ring, dtype), dtype) == 0
    core = (slice(ring, -ring), slice(ring, -ring))
    assert int((_bit_view(got[core]) != _bit_view(back[core])).sum()) > 0
    if hold == 15:  # the ring is held: input values at every level
        outside = torch.ones(full.shape, dtype=torch.bool)
        outside[core] = False
        assert torch.equal(_bit_view(got)[outside], _bit_view(full)[outside])


def test_block_reference_needs_a_core():
    with pytest.raises(ValueError):
        ops.stencil5_exact_block_reference(_field((6, 9), "f32", 1), 3)


def test_periodic_reference_folds_a_one_row_torus():
    """H = 1: rows -1 and H are the row itself."""
    u = _field((1, 4), "f64", 13)
    v = u.tolist()[0]
    want = [[_cell(v[x], v[x], v[x], v[(x - 1) % 4], v[(x + 1) % 4], 0.3, 0.15, "f64") for x in range(4)]]
    assert _differing(ops.stencil5_exact_periodic_reference(u, 1, 0.3, 0.15), want, "f64") == 0


@pytest.mark.parametrize("radius", [1, 2])
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_box_reference_equals_rational_arithmetic(dtype, radius):
    k = 2 * radius + 1
    wts = [0.01 * (i + 1) for i in range(k * k)]
    full = _field((H + 2 * radius, W + 2 * radius), dtype, 14)
    got = ops.box_exact_reference(full, wts)
    v = full.double().tolist()
    w32 = [Fraction(_round(Fraction(w), "f32")) for w in wts]
    want = []
    for y in range(H):
        row = []
        for x in range(W):
            acc = Fraction(0)
            for ky in range(k):
                for kx in range(k):
                    acc = Fraction(_round(w32[ky * k + kx] * Fraction(v[y + ky][x + kx]) + acc, dtype))
            row.append(float(acc))
        want.append(row)
    assert _differing(got, want, dtype) == 0


def test_exact_references_differ_from_the_loose_ones_somewhere():
    """The point of the exact forms: over a few thousand fp64 cells the unfused
    reference (ops.stencil5_reference's expression) is not bitwise the fma."""
    full = _field((66, 66), "f64", 15)
    loose = 0.15 * ((full[:-2, 1:-1] + full[2:, 1:-1]) + (full[1:-1, :-2] + full[1:-1, 2:])) + 0.3 * full[1:-1, 1:-1]
    exact = ops.stencil5_exact_reference(full, 0.3, 0.15)
    assert 0 < int((loose != exact).sum())
    assert torch.allclose(loose, exact, rtol=1e-15, atol=1e-15)


def test_public_fma_is_the_private_one():
    from cuda_mpi_scratch_amd.ops import relaxation

    assert relaxation.fma is relaxation._fma is ops.fma
