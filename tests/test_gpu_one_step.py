"""The one-step kernels (csrc/kernels/stencil_sweep.hpp) and the halo copy, bit
for bit against the exact references of ops/exact.py, at the shapes where each
kernel takes another path.

Conventions of every stencil test here: tiles come from TileGeom.aligned; the
alignment padding of the source is NaN (for the 5-point kernels the four ghost
corners too, which they never read); the destination is pre-filled with a
sentinel. Each check asserts zero differing cells, all stored cells finite,
the sentinel everywhere outside the written rectangle, the source unchanged bit
for bit and the dispatch name. Fields are in [-1, 1].

With N = 16 / sizeof(T) (cells per 16-byte vector) a wave owns a segment of
64 N columns and a register-roll workgroup 256 N columns."""
import pytest
import torch

from cuda_mpi_scratch_amd import core, hip, ops
from cuda_mpi_scratch_amd.models.stencil2d import Stencil2D, StencilConfig
from cuda_mpi_scratch_amd.parallel.halo import NativeHalo, TorchHalo

pytestmark = pytest.mark.gpu

DT = {"f32": torch.float32, "f64": torch.float64}
BITS = {torch.float32: torch.int32, torch.float64: torch.int64}
SENTINEL = -3.0
C_PLAIN = (0.3, 0.15)
C_CHEB = (-37.25, 9.5)  # the size of a Chebyshev level's pair
_CACHE = {}


def _n(dtype):
    return 16 // DT[dtype].itemsize


def _threshold(dtype):
    """First width at which stencil5_rows / stencil5_periodic take four-row strips."""
    return 131072 // DT[dtype].itemsize


def _geom(w, h, dtype, halo=1):
    return core().TileGeom.aligned(w, h, halo, halo, DT[dtype].itemsize)


def _full(buf, g):
    return buf.view(g.total_height(), g.pitch)[:, g.x_origin:g.x_origin + g.total_width()]


def _core(buf, g):
    return _full(buf, g)[g.halo_y:g.halo_y + g.height, g.halo_x:g.halo_x + g.width]


def _field(w, h, dtype, halo=1):
    """Per shape and type, made once and left unchanged: the logical tile (core +
    ghost ring), random in [-1, 1], on the CPU."""
    key = ("field", w, h, dtype, halo)
    if key not in _CACHE:
        gen = torch.Generator(device="cpu").manual_seed(1000 * (w % 9973) + 10 * h + halo)
        _CACHE[key] = (torch.rand(h + 2 * halo, w + 2 * halo, generator=gen, dtype=torch.float64) * 2 - 1).to(DT[dtype])
    return _CACHE[key]


def _want5(w, h, dtype, coeffs=C_PLAIN):
    key = ("want5", w, h, dtype, coeffs)
    if key not in _CACHE:
        _CACHE[key] = ops.stencil5_exact_reference(_field(w, h, dtype), *coeffs)
    return _CACHE[key]


def _want_box(w, h, dtype, radius):
    key = ("wantbox", w, h, dtype, radius)
    if key not in _CACHE:
        _CACHE[key] = ops.box_exact_reference(_field(w, h, dtype, radius), _box_weights(radius))
    return _CACHE[key]


def _box_weights(radius):
    k = 2 * radius + 1
    return [0.01 * (i + 1) for i in range(k * k)]  # asymmetric weights catch transposes


def _source(gpu, g, full, nan_corners):
    """A device tile whose padding is NaN and whose logical tile is `full`."""
    t = torch.full((g.alloc_elems(),), float("nan"), dtype=full.dtype, device=gpu)
    f = _full(t, g)
    f.copy_(full)
    if nan_corners:
        f[0, 0] = f[0, -1] = f[-1, 0] = f[-1, -1] = float("nan")
    return t


def _same_bits(a, b):
    return torch.equal(a.view(BITS[a.dtype]), b.view(BITS[b.dtype]))


def _assert_rect(out, g, rect, want, what):
    """Core rectangle rect = (x0, x1, y0, y1) of `out` equals `want` bit for bit and
    is finite; every other element of the allocation still holds the sentinel."""
    x0, x1, y0, y1 = rect
    have = _core(out, g)[y0:y1, x0:x1].cpu()
    n = int((have != want).sum())
    print(f"{what}: {n} of {have.numel()} cells differ from the reference")
    assert have.numel() == (x1 - x0) * (y1 - y0) > 0
    assert torch.isfinite(have).all(), "a NaN from a corner or from padding reached a stored cell"
    assert n == 0
    rest = out.clone()
    _core(rest, g)[y0:y1, x0:x1] = SENTINEL
    assert bool((rest == SENTINEL).all()), "the kernel wrote outside its rectangle"


def _run5(gpu, dtype, w, h, rect, launch, dispatch, what, coeffs=C_PLAIN):
    g = _geom(w, h, dtype)
    src = _source(gpu, g, _field(w, h, dtype), nan_corners=True)
    before = src.clone()
    dst = torch.full_like(src, SENTINEL)
    launch(src, dst, g)
    torch.cuda.synchronize()
    assert hip().last_stencil_dispatch() == dispatch
    x0, x1, y0, y1 = rect
    _assert_rect(dst, g, rect, _want5(w, h, dtype, coeffs)[y0:y1, x0:x1], f"{what} {dtype} {w}x{h} {rect}")
    assert _same_bits(src, before), "the kernel changed its source"


def _row_ranges(h):
    """The whole core, then the sub-ranges [1, h - 1) and [h - 1, h) where not empty."""
    return [r for r in [(0, h), (1, h - 1), (h - 1, h)] if r[1] > r[0]]


def _rows(gpu, dtype, w, h, variant, coeffs=C_PLAIN, ranges=None):
    for r0, r1 in ranges or _row_ranges(h):
        _run5(gpu, dtype, w, h, (0, w, r0, r1),
              lambda s, d, g: ops.stencil5(s, d, g, r0, r1, coeffs[0], coeffs[1], variant=variant),
              variant, f"stencil5_rows {variant} rows [{r0}, {r1})", coeffs)


# -------------------------------------------------------------- register roll
ROLL3_WIDTHS = {"1": lambda N: 1, "N-1": lambda N: N - 1, "N": lambda N: N, "N+1": lambda N: N + 1,
                "64N-1": lambda N: 64 * N - 1, "64N": lambda N: 64 * N, "64N+1": lambda N: 64 * N + 1,
                "256N": lambda N: 256 * N, "256N+1": lambda N: 256 * N + 1, "256N+64N": lambda N: 320 * N}


@pytest.mark.parametrize("width", list(ROLL3_WIDTHS))
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_roll_three_row_strips(gpu, dtype, width):
    """Three-row strips: height 3 is one full strip, 1 and 2 a ragged one, 4 and 7
    full strips and a ragged one (7 fills the workgroup row of one wave per strip).
    Widths: below, at and past one vector; one column short of, at and past a wave
    segment (lane 63 loads the right edge only when the next segment exists); one
    workgroup, one more column, one more segment."""
    w = ROLL3_WIDTHS[width](_n(dtype))
    for h in (1, 2, 3, 4, 7):
        _rows(gpu, dtype, w, h, "roll")


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_roll_three_row_strips_with_a_chebyshev_sized_pair(gpu, dtype):
    _rows(gpu, dtype, 64 * _n(dtype) + 1, 7, "roll", C_CHEB)


@pytest.mark.parametrize("extra", ["0", "N+1"])
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_roll_four_row_strips(gpu, dtype, extra):
    """From width * sizeof(T) = 131072 on, stencil5_rows takes four-row strips:
    height 4 is one full strip, 1 a ragged one, 5 and 9 full strips and a ragged
    row. The second width ends in a partial vector past the threshold."""
    w = _threshold(dtype) + (0 if extra == "0" else _n(dtype) + 1)
    for h in (1, 4, 5, 9):
        _rows(gpu, dtype, w, h, "roll", ranges=[(0, h)])
    _rows(gpu, dtype, w, 9, "roll", ranges=[(1, 8), (8, 9)])


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_roll_just_below_the_four_row_threshold(gpu, dtype):
    """One column narrower: the three-row form (a full strip and a ragged one at
    height 5), the same exact result. Pins the switch between the two forms."""
    _rows(gpu, dtype, _threshold(dtype) - 1, 5, "roll")


# ------------------------------------------------------------------ LDS tile
LDS_WIDTHS = {"1": lambda N: 1, "N+1": lambda N: N + 1, "64N-1": lambda N: 64 * N - 1, "64N": lambda N: 64 * N,
              "64N+1": lambda N: 64 * N + 1, "128N+3": lambda N: 128 * N + 3}


@pytest.mark.parametrize("width", list(LDS_WIDTHS))
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_lds_tiles(gpu, dtype, width):
    """A workgroup stages a 64 N x 16 tile: heights below, one short of, at and
    past one tile, and two tiles and a row; at 33 also a row range that starts and
    ends inside a 16-row tile."""
    w = LDS_WIDTHS[width](_n(dtype))
    for h in (1, 15, 16, 17, 33):
        _rows(gpu, dtype, w, h, "lds", ranges=[(0, h)])
    _rows(gpu, dtype, w, 33, "lds", ranges=[(3, 11), (1, 32), (32, 33)])


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_lds_tiles_with_a_chebyshev_sized_pair(gpu, dtype):
    _rows(gpu, dtype, 64 * _n(dtype) + 1, 17, "lds", C_CHEB)


# ----------------------------------------------------------------- rectangle
def _rect(gpu, dtype, w, h, rect, coeffs=C_PLAIN):
    x0, x1, y0, y1 = rect
    _run5(gpu, dtype, w, h, rect, lambda s, d, g: ops.stencil5_rect(s, d, g, x0, x1, y0, y1, *coeffs), "rect",
          "stencil5_rect", coeffs)


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_rect_columns_cell_and_interior(gpu, dtype):
    w, h = 37, 11
    _rect(gpu, dtype, w, h, (0, 1, 0, h))          # the first column
    _rect(gpu, dtype, w, h, (w - 1, w, 0, h))      # the last column
    _rect(gpu, dtype, w, h, (5, 6, 3, 4))          # one cell
    _rect(gpu, dtype, w, h, (3, 20, 1, 8))         # interior, odd offsets
    _rect(gpu, dtype, w, h, (3, 20, 1, 8), C_CHEB)


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_rect_second_stride_iteration(gpu, dtype):
    """The grid is capped at 8 workgroups of 256 threads per CU: 1024 cells more
    than that, so the first 1024 threads run the stride loop twice."""
    cells = 8 * hip().device_cu_count() * 256 + 1024
    w = 1024
    h = cells // w
    assert w * h == cells
    _rect(gpu, dtype, w, h, (0, w, 0, h))


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_frame_decomposition_is_bitwise(gpu, dtype):
    """Interior rows on the roll kernel, the two edge columns on rect, then the
    first and the last row: together the whole core, bit for bit."""
    w, h = 520, 64
    g = _geom(w, h, dtype)
    src = _source(gpu, g, _field(w, h, dtype), nan_corners=True)
    before = src.clone()
    dst = torch.full_like(src, SENTINEL)
    c0, c1 = C_PLAIN
    for launch, name in [(lambda: ops.stencil5(src, dst, g, 1, h - 1, c0, c1), "roll"),
                         (lambda: ops.stencil5_rect(src, dst, g, 0, 1, 1, h - 1, c0, c1), "rect"),
                         (lambda: ops.stencil5_rect(src, dst, g, w - 1, w, 1, h - 1, c0, c1), "rect"),
                         (lambda: ops.stencil5(src, dst, g, 0, 1, c0, c1), "roll"),
                         (lambda: ops.stencil5(src, dst, g, h - 1, h, c0, c1), "roll")]:
        launch()
        assert hip().last_stencil_dispatch() == name
    torch.cuda.synchronize()
    _assert_rect(dst, g, (0, w, 0, h), _want5(w, h, dtype), f"frame decomposition {dtype} {w}x{h}")
    assert _same_bits(src, before)


# ----------------------------------------------------------------------- box
def _box(gpu, dtype, radius, w, h, rect):
    g = _geom(w, h, dtype, radius)
    src = _source(gpu, g, _field(w, h, dtype, radius), nan_corners=False)  # the box reads the ring's corners
    before = src.clone()
    dst = torch.full_like(src, SENTINEL)
    x0, x1, y0, y1 = rect
    ops.stencil_box(src, dst, g, x0, x1, y0, y1, _box_weights(radius))
    torch.cuda.synchronize()
    assert hip().last_stencil_dispatch() == "box"
    _assert_rect(dst, g, rect, _want_box(w, h, dtype, radius)[y0:y1, x0:x1], f"box R={radius} {dtype} {w}x{h} {rect}")
    assert _same_bits(src, before), "the kernel changed its source"


@pytest.mark.parametrize("radius", [1, 2])
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_box_whole_cores(gpu, dtype, radius):
    """A workgroup owns 64 x 16 outputs, a thread four rows of one column: one
    cell; one short of, at and past one tile; 3 x 3 tiles with ragged last ones."""
    for w, h in [(1, 1), (63, 15), (64, 16), (65, 17), (129, 35)]:
        _box(gpu, dtype, radius, w, h, (0, w, 0, h))


@pytest.mark.parametrize("radius", [1, 2])
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_box_sub_rectangles(gpu, dtype, radius):
    """Rectangles at (x0, y0) = (5, 3) inside a 75 x 25 core: the staging guard and
    the stores are relative to the rectangle, not the core. Heights 3, 5 and 18
    end a thread's four-row loop midway; 18 and width 65 need a second tile."""
    w, h, x0, y0 = 75, 25, 5, 3
    for rw in (1, 64, 65):
        for rh in (1, 3, 5, 16, 18):
            _box(gpu, dtype, radius, w, h, (x0, x0 + rw, y0, y0 + rh))


# ------------------------------------------------------------ periodic wrap
WRAP_SHAPES = {"N x 1": lambda N, T: (N, 1), "N x 2": lambda N, T: (N, 2), "2N x 3": lambda N, T: (2 * N, 3),
               "64N x 4": lambda N, T: (64 * N, 4), "65N x 5": lambda N, T: (65 * N, 5),
               "300 x 44": lambda N, T: (300, 44), "260 x 7": lambda N, T: (260, 7),
               "T x 4": lambda N, T: (T, 4), "T x 6": lambda N, T: (T, 6)}


@pytest.mark.parametrize("steps", [1, 3])
@pytest.mark.parametrize("shape", list(WRAP_SHAPES))
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_roll_wrap_through_the_solver(gpu, dtype, shape, steps):
    """stencil5_periodic has no binding of its own: a 1 x 1 periodic Stencil2D with
    time_block = 1 launches it once per step (asserted through last_run_blocks).
    Heights 1 and 2 are below one strip (rows -1 and H fold onto core rows), a
    width of N makes one lane both wrap lanes, 3 is one full strip, 4 / 5 / 7 / 44
    end in a ragged strip under wrap, 65 N columns put the right wrap lane in a
    second wave; from the threshold width T on the strips are four rows (4: full,
    6: full and ragged). The ghost ring and the padding of the source are NaN and
    stay so: the kernel reads and writes core cells only."""
    dt = DT[dtype]
    w, h = WRAP_SHAPES[shape](_n(dtype), _threshold(dtype))
    c0, c1 = C_PLAIN
    st = Stencil2D(StencilConfig(global_width=w, global_height=h, dims="1x1", dtype=dtype, seed=4, time_block=1,
                                 fuse_periodic=True, sum_form=False, c_center=c0, c_neighbor=c1))
    assert st.solver.fused_periodic() and st.time_block == 1
    g = st.geom
    start = ops.random_values(0, 0, w, h, w, 4, dtype=dt)
    key = ("wrap", w, h, dtype, steps)
    if key not in _CACHE:
        _CACHE[key] = ops.stencil5_exact_periodic_reference(start, steps, c0, c1)
    st.synchronize()
    cur = st.current()
    other = st.b if cur is st.a else st.a
    assert torch.equal(_core(cur, g).cpu(), start), "fill_random and random_values differ"
    held = _core(cur, g).clone()
    cur.fill_(float("nan"))
    _core(cur, g).copy_(held)
    other.fill_(SENTINEL)
    before = cur.clone()
    torch.cuda.synchronize()
    st.run(steps)
    st.synchronize()
    assert hip().last_stencil_dispatch() == "roll_wrap"
    assert st.last_run_blocks() == [(1, steps)]
    out = st.current()
    assert out is other  # an odd number of steps ends in the other buffer
    _assert_rect(out, g, (0, w, 0, h), _CACHE[key], f"roll_wrap {dtype} {w}x{h} x{steps}")
    if steps == 1:
        assert _same_bits(cur, before), "the kernel changed its source"
    else:  # step 2 stored the source buffer's core, and nothing else of it
        rest = cur.clone()
        _core(rest, g).fill_(float("nan"))
        assert bool(torch.isnan(rest).all()), "a step wrote outside the core"


# ------------------------------------------------------------------ halo copy
@pytest.mark.parametrize("w", [1, 3, 97, 100])
@pytest.mark.parametrize("h", [1, 2, 41])
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_local_halo_copy_equals_the_torch_plan(gpu, dtype, w, h):
    """The one-launch self-exchange of a periodic 1 x 1 plan against TorchHalo over
    the whole allocation, the padding pre-filled with a sentinel. Column segments
    are `depth` wide: depth 4 (fp32) or 2 and 4 (fp64) on a width of whole vectors
    (100) moves them as 16-byte vectors, every other depth and the odd widths one
    element at a time; row segments are vectors only at width 100. make_halo_plan
    refuses no depth, but a ring deeper than the core takes its send bands from
    other copies' destinations, where the result of one concurrent launch is not
    defined: those depths are left out (depth <= min(w, h))."""
    dt = DT[dtype]
    topo = core().CartTopology(1, 1)
    depths = [d for d in (1, 2, 3, 4, 5) if d <= min(w, h)]
    assert depths
    for d in depths:
        g = _geom(w, h, dtype, d)
        plan = core().make_halo_plan(topo, 0, g, True, False)
        assert len(plan.self_copies) == 8 and not plan.sends
        cpu = torch.full((g.alloc_elems(),), SENTINEL, dtype=dt)
        _full(cpu, g).copy_(_field(w, h, dtype, d))
        dev = cpu.to(gpu)
        NativeHalo(plan, "local", None, dtype).exchange(dev)
        TorchHalo(plan).exchange(cpu)
        torch.cuda.synchronize()
        got = dev.cpu()
        n = int((got != cpu).sum())
        print(f"halo copy {dtype} {w}x{h} depth {d}: {n} of {got.numel()} elements differ")
        assert n == 0
        # the exchange did something: the left ghost columns hold the right core columns
        assert torch.equal(_full(got, g)[d:d + h, :d], _core(got, g)[:, w - d:])
