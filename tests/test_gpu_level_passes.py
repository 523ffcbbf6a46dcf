"""The level-table passes of the Chebyshev relaxation (kernels::stencil5_tb_levels,
kernels::stencil5_tb_held_levels; stencil_levels.hip, stencil_pipe_levels.hpp,
stencil_held.hpp) bit for bit: every pipeline form, with and without a
correction tile, every depth, the share walk beyond its defaults, the edges of
the rule that sends a rectangle to the pipeline or to the held tile, and the held
tile on every side, against a CPU reference, with everything a pass may not use
poisoned with NaN. The twin of test_gpu_time_block_depths.py for the kernels
that take one coefficient pair per level.

Reference: ``ops.jacobi_held_levels_reference`` (anchored on the CPU against
rational arithmetic, unequal levels included, in test_one_step_reference_cpu.py).
With no side held it runs on the slice [y0 - S, y1 + S) x [x0 - S, x1 + S) and
its core is the rectangle; with held sides it runs on the whole core-and-ring
array (a cell S + 1 or more from the rectangle cannot reach it in S levels) and
the rectangle is cut out. With a correction tile the rectangle gets one more
rounded add in the element type. Comparisons are on bit patterns.

Every table is the Chebyshev cycle of one fixed 1040 x 160 grid
(``chebyshev_cycle(1040, 160, 0.2, 0.2, S)``), whatever the tile: S unequal
pairs, so a level that takes another level's pair, or the table in another
order, changes the bits (a uniform table cannot see either). With inputs in
[-1, 1] every reference stays finite (about 2 at most), which ``_reference``
asserts.

Every launch (``_check``): a TileGeom.aligned tile with a ring S deep. For fp64
that ring is also all the row padding the wide pipeline asks for: the aligned
layout leads with S rounded up to 2 >= A(S) = S columns for S = 12 and 16, and
its pitch holds the core rounded up to 4 columns plus A(S) (wide_pipe_ok_impl),
so on an aligned geometry whose ring is at least S deep ``wide_pipe_ok`` is never
false for whole 4-cell vectors: no such case exists to pin, and the fp64
rule below is the fp32 rule with 16 columns for 32. The whole input allocation
is NaN except the rectangle and S cells around it; ``corr``, when given, is NaN
outside the rectangle; the output is pre-filled with -3. Asserted: the dispatch
name, the pipeline form where the case intends one, the rectangle equal to the
reference in bits and finite, every other output cell still -3, input and
``corr`` unchanged. The three counts are printed first.

Pipeline forms (pipe_form.hpp: pipe_form_for, per-step form; stencil_pipe.hpp:
with_pipe_form instantiates exactly these), by ``last_pipe_form()``'s
(js0, lag1), js0 = 0 the per-strip layout:

  fp32 S = 20   8 + 12 ascending (8, 3)    below 12288 columns; group 928
                12 + 8 ascending (12, 3)   from 12288 columns (12292 x 24 here); group 912
                12 + 8 descending (12, 0)  set_pipe_lag1(False)
                per strip 11 + 9 (0, 0)    set_pipe_joint(False); group 864
  fp32 S = 24   12 + 12 ascending (12, 3)  group 904; a last group of at most 440 columns is split
                12 + 12 descending (12, 0)
                per strip 13 + 11 (0, 0)   group 832
  fp64 S = 16   8 + 8 ascending (8, 3)     group 944
                8 + 8 descending (8, 0)
                per strip 8 + 8 (0, 0)     group 896
  fp64 S = 12   per strip 6 + 6 (0, 0)     group 928, whatever the switches

11 forms, each with the table alone ("stream_pipe_levels") and with the
correction tile ("stream_pipe_levels_src"): 22 kernels, and
``test_every_pipeline_kernel_was_launched`` asserts that the module launched all
of them. 1040 x 97 is two groups at every form, the last 112 to 208 columns
wide (S = 24: 136 <= 440, split), and 97 rows are no multiple of a 6- or 3-row
block. Under a share of 64 (4 workgroups) 1040 x 301 is 602 group-rows: every
share is longer than the fill, and one crosses from group 0 into group 1 (301
is no multiple of the share).

Which kernel takes a rectangle (stencil_levels.hip: levels_pipe_takes; here
``_takes``): the pipeline if x0 and x1 are multiples of 4, it is wider than 32
columns (fp64 16) and taller than 16 rows; else the held tile with no side
held. An fp32 x0 that is no multiple of 4 is an error (check_block_rect).

Held tile (stencil_held.hpp: HeldShape): rectangles of at most 40 columns (fp64
20) take the narrow tile, else of at most S rows the flat one, else the general
one of 64 (32) columns. Widths of 70 (35) put a ragged last vector beside a held
right side. The frame strips are the solver's (fixed_edge_split with 4-cell
vectors): S rows at the top and bottom, S columns rounded outwards to 4 left and
right; on a tile 262 (fp64 201) columns wide the right strip is 22 (13) columns
and ends in a ragged vector beside the held side.

Not reached at these shapes and left out: pieces of a share beyond the buffer
descriptor's range (kMaxChunkBytes: about 10^5 rows and more of these widths).
"""
import zlib

import pytest
import torch

from cuda_mpi_scratch_amd import core, hip, ops
from tests.source_worker import global_source, make
from tests.test_gpu_time_block_depths import F32, F64, NAME, SENTINEL, _bits, share  # noqa: F401  (share: a fixture)

pytestmark = pytest.mark.gpu

DEPTHS = [(F32, 20), (F32, 24), (F64, 12), (F64, 16)]
DEPTH_IDS = [f"{NAME[d]}-S{S}" for d, S in DEPTHS]
_CACHE = {}
_SEEN = set()  # (dtype name, S, js0, lag1, with corr) of every pipeline launch of the module

# Every form with_pipe_form can pick, as (dtype name, S, js0, lag1).
FORMS = {("f32", 20, 8, 3), ("f32", 20, 12, 3), ("f32", 20, 12, 0), ("f32", 20, 0, 0),
         ("f32", 24, 12, 3), ("f32", 24, 12, 0), ("f32", 24, 0, 0),
         ("f64", 16, 8, 3), ("f64", 16, 8, 0), ("f64", 16, 0, 0),
         ("f64", 12, 0, 0)}
OW = {20: 216, 24: 208, 12: 232, 16: 224}      # 256 - 2 A(S): the columns a strip stores
GROUP = {20: 928, 24: 904, 12: 928, 16: 944}   # columns per group of the default form


def _table(S):
    if ("table", S) not in _CACHE:
        t = core().chebyshev_cycle(1040, 160, 0.2, 0.2, S)
        cen, nei = list(t["center"]), list(t["neighbor"])
        assert len(cen) == len(nei) == S and len(set(zip(cen, nei))) == S  # S unequal pairs
        _CACHE[("table", S)] = (cen, nei)
    return _CACHE[("table", S)]


def _takes(dtype, rect):
    """levels_pipe_takes on an aligned geometry with a ring of at least S (the
    module docstring: wide_pipe_ok holds there, and rows this short fit a chunk)."""
    x0, x1, y0, y1 = rect
    return x0 % 4 == 0 and x1 % 4 == 0 and x1 - x0 > (32 if dtype == F32 else 16) and y1 - y0 > 16


def _rand(shape, *key):
    gen = torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))
    return torch.rand(*shape, generator=gen, dtype=F64) * 2 - 1


def _case(dtype, S, w, h, rect):
    """Geometry; the core-and-ring array, random in [-1, 1] (what the references
    work on; once per tile, never modified); the host image of the input
    allocation (the rectangle and S cells around it in place, NaN everywhere
    else) and of the correction tile (random in [-1, 1] on the rectangle, NaN
    everywhere else)."""
    g = core().TileGeom.aligned(w, h, S, S, 4 if dtype == F32 else 8)
    x0, x1, y0, y1 = rect
    key = ("full", NAME[dtype], S, w, h)
    if key not in _CACHE:
        _CACHE[key] = _rand((g.total_height(), g.total_width()), *key).to(dtype)
    full = _CACHE[key]
    key = ("corr", NAME[dtype], S, w, h, rect)
    if key not in _CACHE:
        _CACHE[key] = _rand((y1 - y0, x1 - x0), *key).to(dtype)
    corr_rect = _CACHE[key]
    assert g.halo_x == g.halo_y == S and 0 <= x0 < x1 <= w and 0 <= y0 < y1 <= h
    ys, xs = slice(y0, y1 + 2 * S), slice(x0, x1 + 2 * S)  # the rectangle and S around it, in core-and-ring coordinates
    rows = torch.full((g.total_height(), g.pitch), float("nan"), dtype=dtype)
    assert g.alloc_elems() == rows.numel() and g.x_origin + g.total_width() <= g.pitch
    rows[ys, g.x_origin + xs.start:g.x_origin + xs.stop] = full[ys, xs]
    corr = torch.full_like(rows, float("nan"))
    oy, ox = g.halo_y, g.x_origin + g.halo_x
    corr[oy + y0:oy + y1, ox + x0:ox + x1] = corr_rect
    return g, full, rows, corr, corr_rect


def _reference(dtype, S, w, h, rect, hold, with_corr):
    """The rectangle after the pass, once per case."""
    key = ("ref", NAME[dtype], S, w, h, rect, hold)
    x0, x1, y0, y1 = rect
    _, full, _, _, corr_rect = _case(dtype, S, w, h, rect)
    if key not in _CACHE:
        cen, nei = _table(S)
        if hold == 0:
            sub = full[y0:y1 + 2 * S, x0:x1 + 2 * S].contiguous()
            ref = ops.jacobi_held_levels_reference(sub, cen, nei, 0)[S:-S, S:-S]
        else:
            ref = ops.jacobi_held_levels_reference(full, cen, nei, hold)[S + y0:S + y1, S + x0:S + x1]
        assert ref.shape == (y1 - y0, x1 - x0) and bool(torch.isfinite(ref).all())
        _CACHE[key] = ref.contiguous()
    if not with_corr:
        return _CACHE[key]
    key = key + ("corr",)
    if key not in _CACHE:
        _CACHE[key] = _CACHE[key[:-1]] + corr_rect  # one rounded add in the element type
        assert bool(torch.isfinite(_CACHE[key]).all())
    return _CACHE[key]


def _check(gpu, dtype, S, w, h, expect, *, rect=None, hold=None, corr=False, form=None, split=None):
    """One launch in the module's common form. hold None: ops.stencil5_tb_levels
    (the pipeline, or the held tile with no side held); else
    ops.stencil5_tb_held_levels. expect: the dispatch name without "_src".
    form: last_pipe_form()'s (js0, lag1); split: its split."""
    H = hip()
    rect = tuple(rect or (0, w, 0, h))
    x0, x1, y0, y1 = rect
    g, _, rows, corr_rows, _ = _case(dtype, S, w, h, rect)
    ref = _reference(dtype, S, w, h, rect, hold or 0, corr)
    cen, nei = _table(S)
    src = rows.reshape(-1).to(gpu)
    cor = corr_rows.reshape(-1).to(gpu) if corr else None
    dst = torch.full_like(src, SENTINEL)
    if hold is None:
        ops.stencil5_tb_levels(src, dst, g, x0, x1, y0, y1, cen, nei, corr=cor)
    else:
        ops.stencil5_tb_held_levels(src, dst, g, x0, x1, y0, y1, cen, nei, hold, corr=cor)
    ran, pf = H.last_stencil_dispatch(), H.last_pipe_form()
    torch.cuda.synchronize()
    if ran.startswith("stream_pipe_levels"):
        _SEEN.add((NAME[dtype], S, pf["js0"], pf["lag1"], corr))
    want = torch.full_like(rows, SENTINEL)
    oy, ox = g.halo_y, g.x_origin + g.halo_x
    inside = torch.zeros(rows.shape, dtype=torch.bool)
    inside[oy + y0:oy + y1, ox + x0:ox + x1] = True
    want[inside] = ref.reshape(-1)
    out = dst.cpu().view(rows.shape)
    diff = _bits(out) != _bits(want)
    n_rect, n_out = int(diff[inside].sum()), int(diff[~inside].sum())
    n_in = int((_bits(src.cpu().view(rows.shape)) != _bits(rows)).sum())
    n_corr = int((_bits(cor.cpu().view(rows.shape)) != _bits(corr_rows)).sum()) if corr else 0
    print(f"{NAME[dtype]} S={S} {w}x{h} rect={rect} hold={hold} corr={corr}: ran {ran} {pf}; {n_rect} of {ref.numel()} "
          f"cells differ, {n_out} cells written outside, {n_in} input cells changed, {n_corr} corr cells changed")
    assert ran == expect + ("_src" if corr else "")
    if form is not None:
        assert (pf["js0"], pf["lag1"]) == tuple(form)
    if split is not None:
        assert pf["split"] == split and H.last_pipe_split() == split
    assert n_rect == 0 and bool(torch.isfinite(out[inside]).all())
    assert n_out == 0, "the pass wrote outside its rectangle"
    assert n_in == 0, "the pass changed its input"
    assert n_corr == 0, "the pass changed its correction tile"


def _levels(gpu, dtype, S, w, h, *, rect=None, corr=False, form=None, split=None):
    """ops.stencil5_tb_levels with the kernel the rule names."""
    r = tuple(rect or (0, w, 0, h))
    _check(gpu, dtype, S, w, h, "stream_pipe_levels" if _takes(dtype, r) else "held_levels", rect=r, corr=corr,
           form=form, split=split)


@pytest.fixture
def switches():
    """The process-wide pipeline switches for one test, restored afterwards."""
    H = hip()
    old = H.pipe_joint(), H.pipe_lag1(), H.pipe_split(), H.pipe_balanced()

    def set_(joint=True, lag1=True, split=True, balanced=True):
        H.set_pipe_joint(joint)
        H.set_pipe_lag1(lag1)
        H.set_pipe_split(split)
        H.set_pipe_balanced(balanced)

    try:
        yield set_
    finally:
        H.set_pipe_joint(old[0])
        H.set_pipe_lag1(old[1])
        H.set_pipe_split(old[2])
        H.set_pipe_balanced(old[3])


# ------------------------------------------------------------------- a. forms
# (dtype, S, w, h, switches off, (js0, lag1), split)
FORM_CASES = [
    (F32, 20, 1040, 97, (), (8, 3), False),
    (F32, 20, 1040, 97, ("lag1",), (12, 0), False),
    (F32, 20, 1040, 97, ("joint",), (0, 0), False),
    (F32, 20, 12292, 24, (), (12, 3), False),  # from kJointWide columns: what a 32768-wide tile takes
    (F32, 24, 1040, 97, (), (12, 3), True),    # 136 columns left for the last group: split
    (F32, 24, 1040, 97, ("split",), (12, 3), False),
    (F32, 24, 1040, 97, ("lag1",), (12, 0), False),
    (F32, 24, 1040, 97, ("joint",), (0, 0), False),
    (F64, 16, 1040, 97, (), (8, 3), False),
    (F64, 16, 1040, 97, ("lag1",), (8, 0), False),
    (F64, 16, 1040, 97, ("joint",), (0, 0), False),
    (F64, 12, 1040, 97, (), (0, 0), False),
    (F64, 12, 1040, 97, ("lag1",), (0, 0), False),
    (F64, 12, 1040, 97, ("joint",), (0, 0), False),
]


def _form_id(c):
    return f"{NAME[c[0]]}-S{c[1]}-{c[2]}x{c[3]}-{'no_' + c[4][0] if c[4] else 'default'}"


def _run_form(gpu, switches, case, corr):
    dtype, S, w, h, off, form, split = case
    switches(**{name: False for name in off})
    _check(gpu, dtype, S, w, h, "stream_pipe_levels", corr=corr, form=form, split=split)


@pytest.mark.parametrize("corr", [False, True], ids=["table", "corr"])
@pytest.mark.parametrize("case", FORM_CASES, ids=_form_id)
def test_every_pipeline_form(gpu, switches, case, corr):
    _run_form(gpu, switches, case, corr)


def test_form_cases_name_every_form():
    """No GPU work: the cases above intend each of the 11 forms at least once."""
    assert {(NAME[c[0]], c[1]) + c[5] for c in FORM_CASES} == FORMS and len(FORMS) == 11


# ------------------------------------------------------------------ b. shares
@pytest.mark.parametrize("corr", [False, True], ids=["table", "corr"])
@pytest.mark.parametrize("balanced", [True, False], ids=["balanced", "equal"])
@pytest.mark.parametrize("dtype,S", DEPTHS, ids=DEPTH_IDS)
def test_long_shares_cross_a_group_boundary(gpu, share, switches, dtype, S, balanced, corr):
    """A GPU shared by 64 processes: 4 workgroups over 2 groups x 301 rows, with
    the fill-aware start table and with equal shares."""
    share(64)
    switches(balanced=balanced)
    blocks = max(1, hip().device_cu_count() // 64)
    assert 2 * 301 > blocks * 100  # every share well beyond the longest fill
    _check(gpu, dtype, S, 1040, 301, "stream_pipe_levels", corr=corr, split=(S == 24))


@pytest.mark.parametrize("corr", [False, True], ids=["table", "corr"])
def test_unsplit_last_group_at_depth_24(gpu, corr):
    """904 + 444 columns: more than the 440 a two-strip group stores, so the last
    group runs whole; 1040 (904 + 136) splits (also in the forms above)."""
    _check(gpu, F32, 24, 904 + 444, 97, "stream_pipe_levels", corr=corr, form=(12, 3), split=False)
    _check(gpu, F32, 24, 1040, 97, "stream_pipe_levels", corr=corr, form=(12, 3), split=True)


# ------------------------------------------------------------------ c. shapes
def _sweep_cases():
    out = []
    for dtype, S in DEPTHS:
        shapes = [(36 if dtype == F32 else 20, 97), (OW[S], 17), (OW[S] + 4, S), (GROUP[S] + 4, S + 1), (OW[S] + 4, 97)]
        out += [pytest.param(dtype, S, w, h, id=f"{NAME[dtype]}-S{S}-{w}x{h}") for w, h in shapes]
    return out


@pytest.mark.parametrize("dtype,S,w,h", _sweep_cases())
def test_shape_sweep(gpu, dtype, S, w, h):
    """Just above the thin widths, exactly one strip, one strip + 4 and one group
    + 4 columns, at 17, S, S + 1 and 97 rows; at most 16 rows is the held tile's."""
    assert _takes(dtype, (0, w, 0, h)) == (h > 16)
    _levels(gpu, dtype, S, w, h)
    _levels(gpu, dtype, S, w, h, corr=True)


def _rule_cases():
    out = []
    for dtype, S in DEPTHS:
        nw = 32 if dtype == F32 else 16
        for what, rect, pipe in (("width-thin", (8, 8 + nw, 3, 100), False),
                                 ("width-thin+4", (8, 12 + nw, 3, 100), True),
                                 ("height-16", (8, 292, 3, 19), False), ("height-17", (8, 292, 3, 20), True),
                                 ("ragged-x1", (8, 290, 3, 100), False)):
            out.append(pytest.param(dtype, S, rect, pipe, id=f"{NAME[dtype]}-S{S}-{what}"))
        if dtype == F64:  # two-cell vectors: x0 = 10 is a vector boundary the pipeline cannot start on
            out.append(pytest.param(dtype, S, (10, 292, 3, 100), False, id=f"{NAME[dtype]}-S{S}-ragged-x0"))
    return out


@pytest.mark.parametrize("dtype,S,rect,pipe", _rule_cases())
def test_rule_edges(gpu, dtype, S, rect, pipe):
    """Rectangles inside a 300 x 104 tile on either side of every edge of the rule."""
    assert _takes(dtype, rect) == pipe
    _levels(gpu, dtype, S, 300, 104, rect=rect)
    _levels(gpu, dtype, S, 300, 104, rect=rect, corr=True)


@pytest.mark.parametrize("S", [20, 24])
def test_f32_rectangles_start_on_a_vector(gpu, S):
    """x0 % 4 = 2 is no fp32 rectangle at all: an error, nothing launched."""
    g, _, rows, _, _ = _case(F32, S, 300, 104, (8, 292, 3, 100))
    src = rows.reshape(-1).to(gpu)
    dst = torch.full_like(src, SENTINEL)
    cen, nei = _table(S)
    with pytest.raises(Exception, match="multiple of the vector width"):
        ops.stencil5_tb_levels(src, dst, g, 10, 292, 3, 100, cen, nei)
    torch.cuda.synchronize()
    assert bool((dst == SENTINEL).all())


@pytest.mark.parametrize("corr", [False, True], ids=["table", "corr"])
@pytest.mark.parametrize("dtype,S", DEPTHS, ids=DEPTH_IDS)
def test_interior_sub_rectangle(gpu, dtype, S, corr):
    """A rectangle strictly inside the core of a 560 x 120 tile, on the pipeline:
    core cells further than S from it are NaN."""
    _check(gpu, dtype, S, 560, 120, "stream_pipe_levels", rect=(8, 540, 5, 110), corr=corr)


# -------------------------------------------------------------- d. held levels
@pytest.mark.parametrize("hold", range(16))
@pytest.mark.parametrize("dtype,S", DEPTHS, ids=DEPTH_IDS)
def test_held_levels_every_hold(gpu, dtype, S, hold):
    w = 70 if dtype == F32 else 35
    _check(gpu, dtype, S, w, 40, "held_levels", hold=hold)
    if hold in (0, 6, 9, 15):
        _check(gpu, dtype, S, w, 40, "held_levels", hold=hold, corr=True)


@pytest.mark.parametrize("shape", ["general", "narrow", "flat"])
@pytest.mark.parametrize("dtype,S", DEPTHS, ids=DEPTH_IDS)
def test_held_levels_tile_shapes(gpu, dtype, S, shape):
    """The rectangles of test_held_tile_is_one_body_for_its_three_sources
    (test_gpu_relaxation.py), at every depth, with unequal levels."""
    w, h, N = (70, 40, 4) if dtype == F32 else (35, 40, 2)
    rect = {"general": (0, w, 0, h), "narrow": (0, N * ((S + N - 1) // N), 0, h), "flat": (0, w, 0, S)}[shape]
    for hold in (0, 15, ops.HOLD_RIGHT):
        _check(gpu, dtype, S, w, h, "held_levels", rect=rect, hold=hold)
        _check(gpu, dtype, S, w, h, "held_levels", rect=rect, hold=hold, corr=True)


def _frame(w, h, S):
    """fixed_edge_split(w, h, S, 4, 15): the four frame strips."""
    xl, xr = (S + 3) // 4 * 4, (w - S) // 4 * 4
    return {"top": (0, w, 0, S), "bottom": (0, w, h - S, h), "left": (0, xl, S, h - S), "right": (xr, w, S, h - S)}


@pytest.mark.parametrize("side", ["top", "bottom", "left", "right"])
@pytest.mark.parametrize("ragged", [False, True], ids=["whole", "ragged"])
@pytest.mark.parametrize("dtype,S", DEPTHS, ids=DEPTH_IDS)
def test_held_levels_frame_strips(gpu, dtype, S, ragged, side):
    w, h = (264, 200) if dtype == F32 else (202, 136)
    if ragged:
        w -= 2 if dtype == F32 else 1
    rect = _frame(w, h, S)[side]
    if ragged and side == "right":
        assert (rect[1] - rect[0]) % (4 if dtype == F32 else 2) != 0
    _check(gpu, dtype, S, w, h, "held_levels", rect=rect, hold=15, corr=True)
    _check(gpu, dtype, S, w, h, "held_levels", rect=rect, hold=15)


# -------------------------------------------------------- e. through the solver
@pytest.mark.parametrize("source", [False, True], ids=["homogeneous", "source"])
@pytest.mark.parametrize("dtype,M", [("f32", 24), ("f64", 12), ("f64", 16)])
def test_solver_cycle_equals_the_torch_backend(gpu, dtype, M, source):
    """One Chebyshev cycle on one rank with fixed edges, the grid of
    test_gpu_relaxation.py's SOLVER: the native passes (the level pipeline inside,
    the held frame around it) against the torch backend, which runs one level per
    iteration through ops.stencil5."""
    args = {"w": 1040, "h": 160, "dtype": dtype, "time_block": M, "seed": 11}
    fields = []
    for backend in ("auto", "torch"):
        st = make(dict(args, backend=backend), source=source)
        assert st.time_block == M and st.cycle == M and (st.solver is None) == (backend == "torch")
        if source:
            st.set_source(global_source(args))
        st.run(M)
        st.synchronize()
        fields.append(st.core_view().cpu().clone())
    n = int((_bits(fields[0]) != _bits(fields[1])).sum())
    print(f"{dtype} M={M} source={source}: {n} of {fields[0].numel()} cells differ from the torch backend's")
    assert n == 0 and bool(torch.isfinite(fields[0]).all())


# ------------------------------------------------------------------- coverage
def test_every_pipeline_kernel_was_launched(gpu, switches):
    """All 11 forms x 2 sources. The forms test above has launched them when the
    module runs whole; what a narrower selection left out is launched here."""
    for case in FORM_CASES:
        for corr in (False, True):
            if (NAME[case[0]], case[1]) + case[5] + (corr,) not in _SEEN:
                _run_form(gpu, switches, case, corr)
                switches()
    want = {f + (corr,) for f in FORMS for corr in (False, True)}
    print(f"pipeline kernels launched: {len(_SEEN & want)} of {len(want)}; others: {sorted(_SEEN - want)}")
    assert _SEEN == want
