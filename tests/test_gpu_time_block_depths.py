"""The uniform time-blocked pass (kernels::stencil5_tb) bit for bit: every depth
of every kernel family against a CPU reference, at small edge shapes, with
everything the pass may not use poisoned with NaN.

References (ops/exact.py, anchored on the CPU in test_one_step_reference_cpu.py
and test_sum_form_reference.py): per step ``stencil5_exact_periodic_reference``
(torus) and ``stencil5_exact_block_reference`` (ghost ring); sum form
``jacobi_sum_reference_global`` (torus) and ``jacobi_sum_block_reference``
(ghost ring). Comparisons are on bit patterns (int32 / int64 views).

Every launch (``_check``): a TileGeom.aligned tile, the ring S deep (no wrap) or
1 deep (wrap); the whole allocation NaN except the cells the pass may use, the
rectangle and S cells around it (no wrap: ring cells deeper than S, the row
padding with the apron columns in it, core cells further than S from a
sub-rectangle are all NaN) or the core (wrap: ghost ring and padding are NaN);
the output pre-filled with -3. Asserted: the dispatch record the case names, the
rectangle equal to the reference and finite, every other cell of the output
allocation still -3, the input unchanged.

Shape numbers (stencil_bodies.hpp StripShape / StreamShape, pipe_form.hpp): a
wave streams a strip of 256 columns (fp64 single-wave kernels: 128) and stores
OW = 256 - 2 A(S) of them, A(S) = S rounded up to the lane vector (4 cells; fp64
single-wave: 2); a workgroup runs a group of 4 strips.

  fp32 two-stage pipeline, one launch (stream_pipe / stream_pipe_sum)
    S        windows    split s0 + s1 (step / sum)     group   fill rows (pipe_fill_rows; step / sum)
    17..19   per strip  S/2+1 + rest / S/2 + rest      864     64, 64, 67 / 61, 67, 70
    20       joint      8 + 12, ascending              928     53
    21..23   per strip                                 832     76, 76, 79 / 73, 79, 82
    24       joint      12 + 12, ascending             904     59  (last group <= 440 columns: split in two)
    25..27   per strip                                 800     88, 88, 91 / 85, 91, 94
    28       joint      12 + 16, descending            896     94
    29..31   per strip  min(S/2+1, 16) + rest / ...    768     91, 94, 97 / 91, 94, 97  (3 rows in flight)
    32       joint      16 + 16, descending            864     100
  1040 x 97: two groups at every depth, the last 112 (S = 20) to 272 (S >= 29)
  columns wide — at S = 24 136 <= 440, so it is split; 97 rows are about one
  fill (53..100) and no multiple of a 6- or 3-row block; 194 group-rows on 256
  workgroups leave most shares one row long or empty. 304 x S (wrap): narrower
  than one group, so the last strips and every apron read wrapped columns,
  some of them twice round the torus, and S rows is the least the launcher
  takes. Under a share of 64 (4 workgroups; 1040 x 301): 602 group-rows, shares
  of ~150 rows, longer than any fill, and one crosses from group 0 into group 1
  in its middle (301 is no multiple of the share).

  fp64 wide-lane pipeline (stream_pipe / stream_pipe_sum), S = 9..16: split
  S/2 + rest, 3 rows in flight, fills of 31, 34, .., 49 rows (16: 39); groups
  of 928 (S <= 12), 896 (13..15) and 944 columns (16: joint 8 + 8, ascending):
  two groups at 1040, the last 96..144 wide. Without wrap it wants A(S) columns of
  row padding left of the core: the aligned layout of a ring of 16 has them at
  every depth (a ring of 9 leads with 10 columns < 12 and would fall back to
  the single-wave kernel), and the ring cells beyond S hold NaN.

  Single-wave stream kernels, S = 1..16. fp32 strips store 248 (S <= 4), 240
  (<= 8), 232 (<= 12), 224 (<= 16) columns; fp64 strips 128 - 2 A(S) = 124 ..
  96. The grid form (stream_grid_rot: fp32 on whole output vectors; stream_grid:
  a ragged x1, and fp64) runs whenever groups x rows < 64 x workgroups, at
  least 512 of them: 520 x 97 is three fp32 strips (the last 24-72 wide) in
  one group and 5-6 fp64 strips in two; 518 is the same with x1 % 4 = 2. fp64
  S >= 9 on whole 4-cell vectors is the wide pipeline's, so those depths reach
  the stream kernel at 518 only. The balanced persistent form needs groups x
  rows >= 64 x workgroups: with the share set to the CU count the launch has
  max(occupancy, 2) <= 8 workgroups, and 1040 x 300 has 2 fp32 groups (5
  strips; 3 fp64 groups), 600 >= 512 group-rows, so every workgroup's share
  is 75 rows or more and half of them cross a group boundary.

  LDS tile (tb_tile): 128 x 32 cells per workgroup (fp64 64 x 32) with
  variant="lds", S <= 8: 300 x 70 is 3 (5) tiles across with a 44-column last
  one and 3 down with a 6-row last one. Thin strips of any variant: at most 32
  (fp64 16) columns -> 32 x 128 tiles (16 x 128, 16 x 64 beyond S = 8); at most
  16 rows -> 128 x 16 (64 x 16) tiles; without wrap only. fp32 beyond S = 16 has
  no thin tile: the pipeline takes the strip.

The shape sweep crosses an apron boundary in every family (S = 4k and 4k + 1)
at 36 columns (fp64 20: just above the thin tile), exactly one strip, one
strip + 4 and one group + 4, with heights 17 (just above the thin tile), S,
S + 1 and 97. Wrapping tiles narrower than a window also have rows shorter
than it (the pitch of a 20-column fp64 torus is 32 elements): the stores of the
last row of a chunk then lie past rows x pitch from the window's first column,
which test_torus_rows_shorter_than_the_window pins at the depths whose apron
pushes them there.
"""
import zlib

import pytest
import torch

from cuda_mpi_scratch_amd import core, hip, ops
from cuda_mpi_scratch_amd.models.stencil2d import Stencil2D, StencilConfig

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
NAME = {F32: "f32", F64: "f64"}
SENTINEL = -3.0
EQ, UNEQ = (0.2, 0.2), (0.5, 0.125)
_CACHE = {}


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == F32 else torch.int64)


def _apron4(s):
    return (s + 3) // 4 * 4


def _case(dtype, S, w, h, wrap, rect, halo):
    """Geometry, the 2-D array of the cells the pass may use (what the reference
    works on; once per case, never modified) and the host image of the input
    allocation: those cells in place, NaN everywhere else."""
    g = core().TileGeom.aligned(w, h, halo, halo, 4 if dtype == F32 else 8)
    x0, x1, y0, y1 = rect
    oy, ox = g.halo_y, g.x_origin + g.halo_x
    if wrap:
        ys, xs = slice(oy, oy + h), slice(ox, ox + w)
    else:
        ys, xs = slice(oy + y0 - S, oy + y1 + S), slice(ox + x0 - S, ox + x1 + S)
    key = ("in", dtype, S, w, h, wrap, rect, halo)
    if key not in _CACHE:
        gen = torch.Generator().manual_seed(zlib.crc32(repr((NAME[dtype],) + key[2:]).encode()))
        _CACHE[key] = torch.rand(ys.stop - ys.start, xs.stop - xs.start, generator=gen, dtype=F64).to(dtype)
    valid = _CACHE[key]
    rows = torch.full((g.total_height(), g.pitch), float("nan"), dtype=dtype)
    assert g.alloc_elems() == rows.numel() and ys.start >= 0 and xs.start >= 0
    assert ys.stop <= g.total_height() and xs.stop <= g.pitch
    rows[ys, xs] = valid
    return g, rows, valid


def _reference(dtype, S, w, h, wrap, rect, halo, sum_form, coeffs):
    """The rectangle after the pass, once per (case, form, coefficients)."""
    key = ("ref", dtype, S, w, h, wrap, rect, halo, sum_form, coeffs)
    if key not in _CACHE:
        _, _, valid = _case(dtype, S, w, h, wrap, rect, halo)
        x0, x1, y0, y1 = rect
        if wrap and sum_form:
            ref = ops.jacobi_sum_reference_global(valid, S, coeffs[0])[y0:y1, x0:x1]
        elif wrap:
            ref = ops.stencil5_exact_periodic_reference(valid, S, *coeffs)[y0:y1, x0:x1]
        elif sum_form:
            ref = ops.jacobi_sum_block_reference(valid, S, coeffs[0])  # x0 % 4 == 0: the rectangle starts even
        else:
            ref = ops.stencil5_exact_block_reference(valid, S, *coeffs)
        assert ref.shape == (y1 - y0, x1 - x0) and bool(torch.isfinite(ref).all())
        _CACHE[key] = ref.contiguous()
    return _CACHE[key]


def _check(gpu, dtype, S, w, h, expect, *, wrap, sum_form=False, coeffs=EQ, rect=None, halo=None, variant="auto",
           ref_sum=None):
    """One stencil5_tb launch in the module's common form. ref_sum: the form of
    the reference where it is not the request's (kernels that run a sum-form
    request per step)."""
    H = hip()
    rect = tuple(rect or (0, w, 0, h))
    halo = halo or (1 if wrap else S)
    g, rows, _ = _case(dtype, S, w, h, wrap, rect, halo)
    ref = _reference(dtype, S, w, h, wrap, rect, halo, sum_form if ref_sum is None else ref_sum, coeffs)
    x0, x1, y0, y1 = rect
    src = rows.reshape(-1).to(gpu)
    dst = torch.full_like(src, SENTINEL)
    H.stencil5_tb(src.data_ptr(), dst.data_ptr(), g, S, x0, x1, y0, y1, coeffs[0], coeffs[1], wrap, NAME[dtype],
                  torch.cuda.current_stream().cuda_stream, variant, sum_form, -1.0)
    ran = H.last_stencil_dispatch()
    torch.cuda.synchronize()
    want = torch.full_like(rows, SENTINEL)
    oy, ox = g.halo_y, g.x_origin + g.halo_x
    inside = torch.zeros(rows.shape, dtype=torch.bool)
    inside[oy + y0:oy + y1, ox + x0:ox + x1] = True
    want[inside] = ref.reshape(-1)
    out = dst.cpu().view(rows.shape)
    diff = _bits(out) != _bits(want)
    n_rect, n_out = int(diff[inside].sum()), int(diff[~inside].sum())
    n_in = int((_bits(src.cpu().view(rows.shape)) != _bits(rows)).sum())
    print(f"{NAME[dtype]} S={S} {w}x{h} rect={rect} wrap={wrap} sum={sum_form} c={coeffs} {variant}: ran {ran}; "
          f"{n_rect} of {ref.numel()} cells differ, {n_out} cells written outside, {n_in} input cells changed")
    assert ran == expect
    assert n_rect == 0 and bool(torch.isfinite(out[inside]).all())
    assert n_out == 0, "the pass wrote outside its rectangle"
    assert n_in == 0, "the pass changed its input"


@pytest.fixture
def share():
    """set_gpu_share for one test, restored afterwards."""
    H = hip()
    old = H.gpu_share()
    try:
        yield H.set_gpu_share
    finally:
        H.set_gpu_share(old)


def _pipe(sum_form):
    return "stream_pipe_sum" if sum_form else "stream_pipe"


FORMS = {"step": (False, EQ), "step_uneq": (False, UNEQ), "sum": (True, EQ)}


# ------------------------------------------------------------------ 1. depths
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("wrap", [False, True], ids=["ring", "wrap"])
@pytest.mark.parametrize("S", range(17, 33))
def test_f32_pipeline_every_depth(gpu, S, wrap, form):
    sum_form, coeffs = FORMS[form]
    _check(gpu, F32, S, 1040, 97, _pipe(sum_form), wrap=wrap, sum_form=sum_form, coeffs=coeffs)


@pytest.mark.parametrize("form", ["step", "sum"])
@pytest.mark.parametrize("S", range(17, 33))
def test_f32_pipeline_every_depth_narrow_torus(gpu, S, form):
    sum_form, coeffs = FORMS[form]
    _check(gpu, F32, S, 304, S, _pipe(sum_form), wrap=True, sum_form=sum_form, coeffs=coeffs)


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("wrap", [False, True], ids=["ring", "wrap"])
@pytest.mark.parametrize("S", range(9, 17))
def test_f64_pipeline_every_depth(gpu, S, wrap, form):
    sum_form, coeffs = FORMS[form]
    _check(gpu, F64, S, 1040, 97, _pipe(sum_form), wrap=wrap, sum_form=sum_form, coeffs=coeffs,
           halo=None if wrap else 16)


@pytest.mark.parametrize("form", ["step", "sum"])
@pytest.mark.parametrize("S", range(9, 17))
def test_f64_pipeline_every_depth_narrow_torus(gpu, S, form):
    sum_form, coeffs = FORMS[form]
    _check(gpu, F64, S, 304, S, _pipe(sum_form), wrap=True, sum_form=sum_form, coeffs=coeffs)


@pytest.mark.parametrize("wrap", [False, True], ids=["ring", "wrap"])
@pytest.mark.parametrize("S", range(1, 17))
def test_f32_stream_grid_every_depth(gpu, S, wrap):
    """Whole vectors: the rotated grid form, and a sum-form request runs it per
    step all the same; x1 = 518: the natural grid form (on the torus the tile
    stays 520 wide, a whole number of vectors)."""
    _check(gpu, F32, S, 520, 97, "stream_grid_rot", wrap=wrap)
    _check(gpu, F32, S, 520, 97, "stream_grid_rot", wrap=wrap, sum_form=True, ref_sum=False)
    if wrap:
        _check(gpu, F32, S, 520, 97, "stream_grid", wrap=True, coeffs=UNEQ, rect=(0, 518, 0, 97))
    else:
        _check(gpu, F32, S, 518, 97, "stream_grid", wrap=False, coeffs=UNEQ)


@pytest.mark.parametrize("wrap", [False, True], ids=["ring", "wrap"])
@pytest.mark.parametrize("S", range(1, 17))
def test_f64_stream_grid_every_depth(gpu, S, wrap):
    """fp64 runs the natural grid form per step; from S = 9 only where the wide
    pipeline cannot (x1 % 4 != 0)."""
    _check(gpu, F64, S, 518, 97, "stream_grid", wrap=wrap, coeffs=UNEQ)
    _check(gpu, F64, S, 518, 97, "stream_grid", wrap=wrap, sum_form=True, ref_sum=False)
    if S <= 8:
        _check(gpu, F64, S, 520, 97, "stream_grid", wrap=wrap)


BW, BH = 1040, 300  # the balanced kernels' tile: 2 fp32 groups (3 fp64) x 300 rows on at most 8 workgroups


@pytest.mark.parametrize("wrap", [False, True], ids=["ring", "wrap"])
@pytest.mark.parametrize("S", range(1, 17))
def test_f32_balanced_rot_every_depth(gpu, share, S, wrap):
    share(hip().device_cu_count())
    _check(gpu, F32, S, BW, BH, "stream_balanced_rot", wrap=wrap, coeffs=EQ if wrap else UNEQ)
    if S > 1:
        _check(gpu, F32, S, BW, BH, "stream_balanced_rot_sum", wrap=wrap, sum_form=True)


@pytest.mark.parametrize("wrap", [False, True], ids=["ring", "wrap"])
@pytest.mark.parametrize("S", range(1, 17))
def test_f32_balanced_ragged_every_depth(gpu, share, S, wrap):
    """x1 % 4 = 2: the natural balanced kernel, per step whatever the request."""
    share(hip().device_cu_count())
    rect = (0, BW - 2, 0, BH)
    if wrap:
        _check(gpu, F32, S, BW, BH, "stream_balanced", wrap=True, sum_form=True, ref_sum=False, rect=rect)
    else:
        _check(gpu, F32, S, BW - 2, BH, "stream_balanced", wrap=False, sum_form=True, ref_sum=False)


@pytest.mark.parametrize("wrap", [False, True], ids=["ring", "wrap"])
@pytest.mark.parametrize("S", range(1, 17))
def test_f64_balanced_every_depth(gpu, share, S, wrap):
    """S <= 8 on whole vectors; deeper blocks at a width the wide pipeline cannot take."""
    share(hip().device_cu_count())
    _check(gpu, F64, S, BW if S <= 8 else BW - 2, BH, "stream_balanced", wrap=wrap, coeffs=UNEQ if wrap else EQ)


@pytest.mark.parametrize("form", ["step", "sum"])
@pytest.mark.parametrize("wrap", [False, True], ids=["ring", "wrap"])
@pytest.mark.parametrize("S", [17, 21, 25, 29])  # one depth per apron class
def test_f32_pipeline_long_shares(gpu, share, S, wrap, form):
    """A GPU shared by 64 processes: 4 workgroups over 2 groups x 301 rows, every
    share longer than the fill, the middle one across the group boundary."""
    share(64)
    sum_form, coeffs = FORMS[form]
    _check(gpu, F32, S, 1040, 301, _pipe(sum_form), wrap=wrap, sum_form=sum_form, coeffs=coeffs)


@pytest.mark.parametrize("wrap", [False, True], ids=["ring", "wrap"])
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("S", range(1, 9))
def test_lds_variant_every_depth(gpu, S, dtype, wrap):
    _check(gpu, dtype, S, 300, 70, "tb_tile", wrap=wrap, variant="lds", coeffs=UNEQ if S % 2 else EQ)


# ------------------------------------------------------------------ 2. shapes
SWEEP_DEPTHS = {F32: (8, 9, 16, 17, 20, 21, 24, 32), F64: (8, 9, 12, 13, 16)}


def _strip(dtype, S):
    """Output columns of one strip of the family that runs <dtype, S> on whole vectors."""
    if dtype == F64 and S <= 8:
        return 128 - 2 * ((S + 1) // 2 * 2)
    return 256 - 2 * _apron4(S)


def _sweep_kernel(dtype, S, wrap, w, h, sum_form=False):
    """stencil.hip launch_tb / dispatch_tb on whole vectors: fp32 beyond 16 is the
    pipeline's; thin rectangles (no wrap) the LDS tile's; fp64 from 9 the wide
    pipeline's; the rest the grid form's (small tiles)."""
    if dtype == F32 and S > 16:
        return _pipe(sum_form)
    if not wrap and (w <= (32 if dtype == F32 else 16) or h <= 16):
        return "tb_tile"
    if dtype == F64 and S >= 9:
        return _pipe(sum_form)
    return "stream_grid_rot" if dtype == F32 else "stream_grid"


def _sweep_cases():
    out = []
    for dtype in (F32, F64):
        for S in SWEEP_DEPTHS[dtype]:
            ow = _strip(dtype, S)
            shapes = [(36 if dtype == F32 else 20, 97), (ow, 17), (ow + 4, S), (4 * ow + 4, S + 1), (ow + 4, 97)]
            for w, h in shapes:
                for wrap in (False, True):
                    if wrap and h < S:
                        continue
                    name = f"{NAME[dtype]}-S{S}-{w}x{h}-{'wrap' if wrap else 'ring'}"
                    out.append(pytest.param(dtype, S, w, h, wrap, id=name))
    return out


@pytest.mark.parametrize("dtype,S,w,h,wrap", _sweep_cases())
def test_shape_sweep(gpu, dtype, S, w, h, wrap):
    halo = 16 if (dtype == F64 and S >= 9 and not wrap) else None
    _check(gpu, dtype, S, w, h, _sweep_kernel(dtype, S, wrap, w, h), wrap=wrap, coeffs=UNEQ, halo=halo)
    name = _sweep_kernel(dtype, S, wrap, w, h, sum_form=True)
    if name == "stream_pipe_sum":
        _check(gpu, dtype, S, w, h, name, wrap=wrap, sum_form=True, halo=halo)


@pytest.mark.parametrize("dtype,S,w,kernel", [
    (F32, 29, 36, "stream_pipe"), (F32, 30, 36, "stream_pipe"), (F32, 31, 36, "stream_pipe"),
    (F32, 13, 52, "stream_grid_rot"), (F32, 16, 52, "stream_grid_rot"),
    (F64, 13, 20, "stream_pipe"), (F64, 14, 20, "stream_pipe"), (F64, 15, 20, "stream_pipe"),
])
def test_torus_rows_shorter_than_the_window(gpu, dtype, S, w, kernel):
    """A wrapping tile has no row padding to speak of: at 36 (52, 20) columns the
    pitch is 64 (64, 32) elements, less than the A(S) + w columns from the
    window's first column to its last stored one. The branch-free stores' range
    must still cover the last row of every chunk (chunk_out_rsrc); 97 rows are
    97 one-row pipeline chunks or two grid chunks."""
    _check(gpu, dtype, S, w, 97, kernel, wrap=True, coeffs=UNEQ)
    if kernel == "stream_pipe":
        _check(gpu, dtype, S, w, 97, "stream_pipe_sum", wrap=True, sum_form=True)


@pytest.mark.parametrize("dtype,S", [pytest.param(d, S, id=f"{NAME[d]}-S{S}") for d in (F32, F64)
                                     for S in SWEEP_DEPTHS[d]])
def test_sub_rectangles(gpu, dtype, S):
    """Rectangles strictly inside the core of a 560 x 120 ghost-ring tile: on
    vector multiples, and with a ragged x1 (depths <= 16: the natural grid form)."""
    halo = 16 if (dtype == F64 and S >= 9) else None
    rect = (8, 540, 5, 110)
    _check(gpu, dtype, S, 560, 120, _sweep_kernel(dtype, S, False, 532, 105), wrap=False, coeffs=UNEQ, rect=rect,
           halo=halo)
    if S <= 16:
        _check(gpu, dtype, S, 560, 120, "stream_grid", wrap=False, rect=(8, 537, 5, 110), halo=halo)
    else:
        _check(gpu, dtype, S, 560, 120, "stream_pipe_sum", wrap=False, sum_form=True, rect=rect)


def _thin_cases():
    out = []
    for dtype in (F32, F64):
        for S in (7, 9, 13, 16) + ((20, 24) if dtype == F32 else ()):
            nw = 32 if dtype == F32 else 16
            for what, rect in (("cols", (8, 8 + nw, 3, 100)), ("rows", (8, 292, 3, 19)),
                               ("cols-4", (8, 8 + nw - 4, 0, 104)), ("rows-1", (0, 300, 89, 104))):
                out.append(pytest.param(dtype, S, rect, id=f"{NAME[dtype]}-S{S}-{what}"))
    return out


@pytest.mark.parametrize("dtype,S,rect", _thin_cases())
def test_thin_strips(gpu, dtype, S, rect):
    """The overlap schedule's boundary strips inside a 300 x 104 ghost-ring tile:
    the thin LDS tiles up to S = 16, the pipeline beyond (fp32)."""
    _check(gpu, dtype, S, 300, 104, "stream_pipe" if S > 16 else "tb_tile", wrap=False, coeffs=UNEQ, rect=rect)


# -------------------------------------------------------- 3. through the solver
@pytest.mark.parametrize("dtype,block,runs,depths", [
    # 16 + 15, 17 + 17, 24 + 23, 19 + 18 + 18, 22 + 22 + 21, 20 + 20 + 20 + 19
    ("f32", 24, (23, 31, 34, 47, 55, 65, 79), range(15, 25)),
    # 10 + 9, 12 + 11, 14 + 13, 16 + 15
    ("f64", 16, (15, 19, 23, 27, 31), range(9, 17)),
])
def test_solver_runs_equal_the_exact_torus(gpu, dtype, block, runs, depths):
    """run(K) on one periodic rank (the fused wrap pass, eager launches, per
    step) against K exact steps; call_plan splits each K near-equally into
    depths that follow one another in one run (the comments above; the test
    takes the split from plan_call and the solver's own record)."""
    w, h = 1040, 128
    seen = set()
    for K in runs:
        st = Stencil2D(StencilConfig(global_width=w, global_height=h, dims="1x1", dtype=dtype, periodic=True,
                                     graph=False, sum_form=False, time_block=block, seed=77))
        assert st.time_block == block
        u0 = st.core_view().cpu().clone()
        plan = [tuple(b) for b in core().plan_call(K, block, "fused")["blocks"]]
        st.run(K)
        st.synchronize()
        assert st.last_run_blocks() == plan and sum(s * n for s, n in plan) == K
        key = ("solver", dtype, K)
        if key not in _CACHE:
            _CACHE[key] = ops.stencil5_exact_periodic_reference(u0, K)
        got = st.core_view().cpu()
        n = int((_bits(got) != _bits(_CACHE[key])).sum())
        print(f"{dtype} run({K}) at block {block}: blocks {plan}, {n} of {got.numel()} cells differ")
        assert n == 0 and bool(torch.isfinite(got).all())
        seen.update(s for s, _ in plan)
    print(f"{dtype}: depths run through the solver: {sorted(seen)}")
    assert set(depths) <= seen  # what the list of K was chosen for
