"""One kernel per multigrid step for the solver (mg_*) and for the V-cycle
preconditioner (mgp_*): with every side a ring the preconditioner's entry gives
the plain entry's bits, step by step. The two are different instantiations of
one kernel, so this holds only if the ghost code of the one folds to nothing in
the other and changes nothing where no side has a code.

Each case runs both entries on the same input tiles (padding NaN) into tiles
that start as a sentinel and compares the whole flat output, ring and padding
included, bit for bit (a zero's sign too)."""
import pytest
import torch

from cuda_mpi_scratch_amd import ops
from tests.test_gpu_cg import _same_bits
from tests.test_gpu_multigrid import DT, SENTINEL, _core, _fields, _geom, _rand, _smooth_table, _tile

pytestmark = pytest.mark.gpu


def _assert_same_tile(plain, precond, g, what):
    torch.cuda.synchronize()
    a, b = plain.cpu(), precond.cpu()
    n = int((a != b).sum())
    print(f"{what}: {n} of {a.numel()} elements differ between the two entries")
    assert torch.isfinite(_core(b, g)).all(), "a NaN from a ring or from padding reached a stored cell"
    assert _same_bits(a, b)
    rest = b.clone()
    _core(rest, g).fill_(SENTINEL)
    assert bool((rest == SENTINEL).all()), "the kernel wrote outside the core"


@pytest.mark.parametrize("nu", [1, 2, 3, 4])
@pytest.mark.parametrize("w,h", [(3, 3), (63, 31), (65, 33), (130, 70)])
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_smoother_on_ring_sides_is_the_plain_smoother(gpu, dtype, w, h, nu):
    """A workgroup stores a 64 x 32 tile: (3, 3) sits inside every apron, (63, 31)
    is one cell under a tile, (65, 33) one cell over it, (130, 70) is 3 x 3 tiles
    with ragged last ones; 1..4 fused sweeps are four instantiations. The start
    from zero is the plain smoother on a zeroed tile."""
    dt = DT[dtype]
    u, gsrc = _fields(w, h, dt)
    ce, nb, wt = _smooth_table(w, h, nu)
    g = _geom(w, h, dt)
    src = _tile(gpu, g, dt, core_vals=gsrc)
    for name, full in (("", u), (" from zero", torch.zeros_like(u))):
        u_in = _tile(gpu, g, dt, full=full)
        plain, precond = _tile(gpu, g, dt, fill=SENTINEL), _tile(gpu, g, dt, fill=SENTINEL)
        ops.mg_smooth(u_in, plain, src, g, ce, nb, wt)
        ops.mgp_smooth(None if name else u_in, precond, src, g, ce, nb, wt)
        _assert_same_tile(plain, precond, g, f"smooth{name} {dtype} {w}x{h} NU={nu}")


TRANSFER = [(3, 3), (63, 31), (131, 259)]  # odd: the coarse level of both rules is ((w - 1) / 2, (h - 1) / 2)


@pytest.mark.parametrize("w,h", TRANSFER)
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_residual_restrict_on_ring_sides_is_the_plain_one(gpu, dtype, w, h):
    """A workgroup owns 32 x 16 coarse cells: one cell, one partial tile, 3 x 9 tiles."""
    dt = DT[dtype]
    u, gsrc = _fields(w, h, dt)
    g, gc = _geom(w, h, dt), _geom(w // 2, h // 2, dt)
    u_t, src = _tile(gpu, g, dt, full=u), _tile(gpu, g, dt, core_vals=gsrc)
    plain, precond = _tile(gpu, gc, dt, fill=SENTINEL), _tile(gpu, gc, dt, fill=SENTINEL)
    ops.mg_residual_restrict(u_t, src, g, plain, gc, 0.2, 0.2)
    ops.mgp_residual_restrict(u_t, src, g, precond, gc, 0.2, 0.2)
    _assert_same_tile(plain, precond, gc, f"residual_restrict {dtype} {w}x{h}")


@pytest.mark.parametrize("w,h", TRANSFER)
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_prolong_add_on_ring_sides_is_the_plain_one(gpu, dtype, w, h):
    dt = DT[dtype]
    u, _ = _fields(w, h, dt)
    g, gc = _geom(w, h, dt), _geom(w // 2, h // 2, dt)
    e = _rand((h // 2, w // 2), torch.Generator(device="cpu").manual_seed(7 * w + h), dt)
    e_t = _tile(gpu, gc, dt, core_vals=e)  # ring and padding NaN: e = 0 outside the core
    plain = _tile(gpu, g, dt, core_vals=u[1:-1, 1:-1], fill=SENTINEL)  # in place
    precond = plain.clone()
    ops.mg_prolong_add(e_t, gc, plain, g)
    ops.mgp_prolong_add(e_t, gc, precond, g)
    _assert_same_tile(plain, precond, g, f"prolong_add {dtype} {w}x{h}")


@pytest.mark.parametrize("w,h", [(1, 1), (16, 8), (63, 63)])
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_coarse_solve_on_ring_sides_is_the_plain_one(gpu, dtype, w, h):
    """One cell, a grid inside one pass of the workgroup's 256 threads, and the
    largest grid (above the default LDS limit in fp64: each instantiation raises
    its own)."""
    dt = DT[dtype]
    p = ops.mg_coarse_plan(w, h, 0.2, 0.2, 1e-3)
    gsrc = _rand((h, w), torch.Generator(device="cpu").manual_seed(w + 64 * h), dt, 1e-3)
    g = _geom(w, h, dt)
    src = _tile(gpu, g, dt, core_vals=gsrc)
    plain, precond = _tile(gpu, g, dt, fill=SENTINEL), _tile(gpu, g, dt, fill=SENTINEL)
    ops.mg_coarse_solve(src, plain, g, p["center"], p["neighbor"], p["weight"], p["repeats"])
    ops.mgp_coarse_solve(src, precond, g, p["center"], p["neighbor"], p["weight"], p["repeats"])
    _assert_same_tile(plain, precond, g, f"coarse_solve {dtype} {w}x{h}")
