"""dot, fill, fill_region and fill_random on the GPU: exact where the data allow
it (one-hot and small-integer dot products, fills against the CPU path of the
same op, fill_random against its CPU twin bit for bit) and a derived rounding
bound where they do not.

dot streams 16-byte vectors: N = 16 / sizeof(T) elements each, 256 threads x 8
vectors per workgroup iteration, so one iteration covers C = 2048 N elements
(a "chunk"). Whole chunks run without bounds checks, one ragged chunk follows,
then a scalar tail of n mod N elements."""
import math

import numpy as np
import pytest
import torch

from cuda_mpi_scratch_amd import core, hip, ops

pytestmark = pytest.mark.gpu

DT = {"f32": torch.float32, "f64": torch.float64}
PAIRS = [("f32", "f32"), ("f32", "f64"), ("f64", "f64")]  # (element type, accumulator)
MODES = ["atomic", "two-pass", "single-pass", "host"]
UNIT_ROUNDOFF = {"f32": 2.0 ** -24, "f64": 2.0 ** -53}
SENTINEL = -3.0
GUARD = 64


def _n(dtype):
    return 16 // DT[dtype].itemsize


def _chunk(dtype):
    return 2048 * _n(dtype)


def _ws(n, gpu, acc, grid=None):
    """A DotWorkspace; with an explicit grid its partials are sized for that grid
    (the default workspace holds one slot per workgroup of the default grid)."""
    ws = ops.DotWorkspace(n, gpu, DT[acc])
    if grid is not None:
        ws.grid = grid
        ws.partials = torch.empty(grid, dtype=DT[acc], device=gpu)
    return ws


def _dot(x, y, mode, acc, ws):
    r = ops.dot(x, y, mode, acc=acc, ws=ws)
    if mode == "host":  # the partials of the launch, summed on the host
        assert r.numel() == ws.grid
        return float(r.double().sum().item())
    return float(r.item())


# ---------------------------------------------------------------- dot, exact
@pytest.mark.parametrize("dtype,acc", PAIRS)
def test_dot_pairs_every_position_with_itself(gpu, dtype, acc):
    """y is one-hot at k, x[i] = (i mod 251) + 1: the result is x[k] exactly, for k
    at both ends of every region. With grid = 2, block 0 takes chunks 0 and 2 (its
    whole-chunk loop strides once), block 1 chunk 1 and the ragged chunk of 777
    vectors (three full rows of 256 lanes and 9 lanes of a fourth), and the tail
    of N - 1 elements falls to the first threads of block 0."""
    N, C = _n(dtype), _chunk(dtype)
    n = 3 * C + 777 * N + (N - 1)
    nvec = n // N
    x = ((torch.arange(n) % 251) + 1).to(DT[dtype]).to(gpu)
    y = torch.zeros(n, dtype=DT[dtype], device=gpu)
    ws = _ws(n, gpu, acc, grid=2)
    ks = [0, N - 1, N, C - 1, C, 2 * C - 1, 2 * C, 3 * C - 1, 3 * C, 3 * C + 256 * N - 1, 3 * C + 256 * N,
          nvec * N - 1, nvec * N, n - 1]
    assert all(0 <= k < n for k in ks) and nvec * N < n
    wrong = []
    for mode in MODES:
        for k in ks:
            y[k] = 1.0
            got = _dot(x, y, mode, acc, ws)
            y[k] = 0.0
            if got != float(k % 251 + 1):
                wrong.append((mode, k, got, k % 251 + 1))
    print(f"dot one-hot {dtype}/{acc} n={n}: {len(wrong)} of {len(MODES) * len(ks)} wrong {wrong[:8]}")
    assert not wrong


def _small_integers(n, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    v = torch.randint(1, 4, (n,), generator=g) * (torch.randint(0, 2, (n,), generator=g) * 2 - 1)
    return v, v.to(DT[dtype])


@pytest.mark.parametrize("dtype,acc", PAIRS)
def test_dot_of_small_integers_is_exact(gpu, dtype, acc):
    """x, y in {+-1, +-2, +-3}: sum |x_i y_i| < 2^24, so every partial sum, in any
    order, is an integer either accumulator holds exactly, and the result is the
    int64 dot product. Sizes: none, below / at / past one vector, one lane short
    of and past one row of lanes, around one chunk, two chunks and a vector and a
    tail; each with the default grid and with 1 and 3 workgroups. The last size
    takes the default grid (one workgroup per CU) through a second stride
    iteration of the whole-chunk loop."""
    N, C = _n(dtype), _chunk(dtype)
    cus = hip().device_cu_count()
    sizes = [0, 1, N - 1, N, N + 1, 256 * N - 1, 256 * N + 1, C - 1, C, C + 1, 2 * C + N + 1]
    cases = [(n, grid) for n in sizes for grid in (None, 1, 3)] + [(cus * C + C + 5, None)]
    wrong = []
    for n, grid in cases:
        xi, x = _small_integers(n, dtype, 2 * n + 1)
        yi, y = _small_integers(n, dtype, 2 * n + 2)
        assert int((xi * yi).abs().sum()) < 2 ** 24
        want = int((xi * yi).sum())
        ws = _ws(n, gpu, acc, grid)
        if grid is None and n == cases[-1][0]:
            assert ws.grid == cus and n // N > ws.grid * 2048  # some workgroup strides twice
        xd, yd = x.to(gpu), y.to(gpu)
        for mode in MODES:
            got = _dot(xd, yd, mode, acc, ws)
            if got != float(want):
                wrong.append((n, grid, mode, got, want))
    print(f"dot small integers {dtype}/{acc}: {len(wrong)} of {len(cases) * len(MODES)} wrong {wrong[:8]}")
    assert not wrong


def test_dot_of_nothing_is_zero(gpu):
    x = torch.empty(0, dtype=torch.float64, device=gpu)
    for mode in MODES:
        ws = _ws(0, gpu, "f64")
        ws.out.fill_(7.0)
        ws.partials.fill_(7.0)
        assert _dot(x, x, mode, "f64", ws) == 0.0


# ------------------------------------------------------------- dot, rounding
def _chain_length(n, grid, mode, dtype):
    """The most rounded additions a product passes through, read off dot.hip:
    the fused multiply-adds into one of a lane's 8 accumulators (N per whole-chunk
    iteration of its workgroup, N in the ragged chunk, one more in the scalar
    tail, which has fewer elements than there are threads), 7 to add the 8
    accumulators, 6 butterfly steps over the wave, 4 to add the waves' LDS slots,
    then the combine step: one atomic add per workgroup; or (two-pass and
    single-pass) a lane's strided sum over the partials and another block sum
    (6 + 4); or the host's sum over the partials."""
    N = _n(dtype)
    whole = (n // N) // 2048
    per_lane = N * (math.ceil(whole / grid) + 1) + 1
    combine = {"atomic": grid, "host": grid}.get(mode, math.ceil(grid / 256) + 10)
    return per_lane + 7 + 6 + 4 + combine


@pytest.mark.parametrize("dtype,acc", PAIRS)
def test_dot_rounding_stays_inside_the_derived_bound(gpu, dtype, acc):
    """Uniform [-1, 1] data against products and sum in numpy.longdouble:
    |got - ref| <= D u sum |x_i y_i| with u the accumulator's unit roundoff and D
    the chain length above. For (f32, acc f64) the bound is one of fp64 sums:
    accumulating in fp32 misses it by orders of magnitude."""
    u = UNIT_ROUNDOFF[acc]
    worst = 0.0
    for n in (2 * _chunk(dtype) + _n(dtype) + 1, 300_001):
        g = torch.Generator().manual_seed(n)
        x = (torch.rand(n, generator=g, dtype=torch.float64) * 2 - 1).to(DT[dtype])
        y = (torch.rand(n, generator=g, dtype=torch.float64) * 2 - 1).to(DT[dtype])
        prod = x.numpy().astype(np.longdouble) * y.numpy().astype(np.longdouble)
        ref, scale = prod.sum(), np.abs(prod).sum()
        xd, yd = x.to(gpu), y.to(gpu)
        for grid in (None, 3):
            ws = _ws(n, gpu, acc, grid)
            for mode in MODES:
                got = _dot(xd, yd, mode, acc, ws)
                D = _chain_length(n, ws.grid, mode, dtype)
                ratio = float(abs(np.longdouble(got) - ref) / (D * u * scale))
                worst = max(worst, ratio)
                print(f"dot rounding {dtype}/{acc} n={n} grid={ws.grid} {mode}: got {got!r}, ref {float(ref)!r}, "
                      f"D={D}, |err| / bound = {ratio:.3g}")
                assert ratio <= 1.0
    print(f"dot rounding {dtype}/{acc}: worst |err| / bound = {worst:.3g}")


def test_dot_refuses_a_narrow_accumulator_and_misaligned_input(gpu):
    x = torch.ones(4099, dtype=torch.float64, device=gpu)
    with pytest.raises(ValueError, match="f64 accumulator"):
        ops.dot(x, x, "two-pass", acc="f32")
    for dtype in (torch.float32, torch.float64):
        a = torch.ones(4099, dtype=dtype, device=gpu)
        assert a.data_ptr() % 16 == 0 and a[1:].data_ptr() % 16 != 0
        with pytest.raises(Exception, match="16-byte aligned"):
            ops.dot(a[1:], a[:-1])
        with pytest.raises(Exception, match="16-byte aligned"):
            ops.dot(a[:-1], a[1:])


# ---------------------------------------------------------- fill, fill_region
def _guarded(elems, dtype, device):
    """A buffer of `elems` elements between two guards, all holding the sentinel;
    returns (whole buffer, the inner view)."""
    buf = torch.full((elems + 2 * GUARD,), SENTINEL, dtype=dtype, device=device)
    return buf, buf[GUARD:GUARD + elems]


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_fill_equals_the_cpu_path(gpu, dtype):
    """Sizes: nothing, one element, one short of / at / past one workgroup, and 3
    elements more than the capped grid covers in one stride."""
    cap = 8 * hip().device_cu_count() * 256
    for n in (0, 1, 255, 256, 257, cap + 3):
        for value in (2.5, 0.1):
            dev, dv = _guarded(n, DT[dtype], gpu)
            cpu, cv = _guarded(n, DT[dtype], "cpu")
            ops.fill(dv, value)
            ops.fill(cv, value)
            torch.cuda.synchronize()
            diff = int((dev.cpu() != cpu).sum())
            print(f"fill {dtype} n={n} value={value}: {diff} of {cpu.numel()} elements differ")
            assert diff == 0
            assert n == 0 or float(cv[0]) != SENTINEL


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_fill_region_equals_the_cpu_path(gpu, dtype):
    A = core().Array2D
    cap = 8 * hip().device_cu_count() * 256
    big_h = cap // 1000 + 2
    cases = [("width-1 column", 12, A(1, 9, 40, 3, 1)),
             ("height-1 row", 12, A(17, 1, 40, 2, 4)),
             ("1 x 1 at an offset", 12, A(1, 1, 40, 5, 7)),
             ("window narrower than the stride", 12, A(20, 6, 40, 4, 2)),
             ("no columns", 12, A(0, 5, 40, 3, 1)),
             ("no rows", 12, A(5, 0, 40, 3, 1)),
             ("above the grid cap", big_h + 3, A(1000, big_h, 1030, 7, 2))]
    assert 1000 * big_h > cap
    for name, rows, region in cases:
        elems = rows * region.row_stride
        dev, dv = _guarded(elems, DT[dtype], gpu)
        cpu, cv = _guarded(elems, DT[dtype], "cpu")
        ops.fill_region(dv, region, 0.7)
        ops.fill_region(cv, region, 0.7)
        torch.cuda.synchronize()
        diff = int((dev.cpu() != cpu).sum())
        written = int((cpu != SENTINEL).sum())
        print(f"fill_region {dtype} {name}: {diff} of {cpu.numel()} elements differ, {written} written")
        assert diff == 0
        assert written == region.width * region.height


# --------------------------------------------------------------- fill_random
# ops.random_values(17, 5, 4, 2, 1000, seed=99) on [0, 1), recorded from the CPU
# twin before the kernel and the twin were made one definition: 24-bit values,
# the same in both types. Every seed-dependent reference of the suite rests on
# these staying put.
RECORDED = [[0.6731213331222534, 0.6245077252388, 0.5740290880203247, 0.3217657804489136],
            [0.5045038461685181, 0.7105934023857117, 0.8378974199295044, 0.19042235612869263]]


@pytest.mark.parametrize("lo,hi", [(0.0, 1.0), (-0.3, 0.9), (2.5, 2.75), (-1e-3, 1e3)])
@pytest.mark.parametrize("w,h", [(1, 1), (300, 41), (257, 3)])
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_fill_random_is_bitwise_the_cpu_twin(gpu, dtype, w, h, lo, hi):
    """value = lo + round(T(u) * span), span = T(hi) - T(lo): two rounded
    operations in the kernel and in the twin, at a non-zero global offset inside a
    wider global grid; the ghost ring and the padding keep the sentinel."""
    dt = DT[dtype]
    g = core().TileGeom.aligned(w, h, 1, 1, dt.itemsize)
    dev = torch.full((g.alloc_elems(),), SENTINEL, dtype=dt, device=gpu)
    cpu = torch.full((g.alloc_elems(),), SENTINEL, dtype=dt)
    ops.fill_random(dev, g, 17, 5, 1000, seed=99, lo=lo, hi=hi)
    ops.fill_random(cpu, g, 17, 5, 1000, seed=99, lo=lo, hi=hi)
    torch.cuda.synchronize()
    got = dev.cpu()
    diff = int((got != cpu).sum())
    print(f"fill_random {dtype} {w}x{h} [{lo}, {hi}): {diff} of {got.numel()} elements differ")
    assert diff == 0
    view = cpu.view(g.total_height(), g.pitch)
    y0, x0 = g.halo_y, g.x_origin + g.halo_x
    core_vals = view[y0:y0 + h, x0:x0 + w].clone()
    assert torch.equal(core_vals, ops.random_values(17, 5, w, h, 1000, 99, lo, hi, dt))
    view[y0:y0 + h, x0:x0 + w] = SENTINEL
    assert bool((cpu == SENTINEL).all()), "the twin wrote outside the core"
    if (lo, hi) == (0.0, 1.0) and (w, h) == (300, 41):
        assert core_vals[:2, :4].double().tolist() == RECORDED
        assert ops.random_values(17, 5, 4, 2, 1000, 99, dtype=dt).double().tolist() == RECORDED
