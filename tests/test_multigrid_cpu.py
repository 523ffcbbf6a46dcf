"""Geometric multigrid without a GPU: the level planner and the sweep tables
(host-only C++ through _mxs_core), the transfer operators' algebra, the
convergence of the reference V-cycle on the prototype's problem, the torch
backend of Multigrid2D and a manufactured Poisson solution with a proven bound."""
import math

import pytest
import torch

from cuda_mpi_scratch_amd import core, ops
from cuda_mpi_scratch_amd.models.multigrid2d import Multigrid2D, MultigridConfig
from tests.test_source_cpu import manufactured

F32, F64 = torch.float32, torch.float64


def prototype(w, h, dtype="f64", **kw):
    """The problem the method was prototyped on: c0 = c1 = 0.2, top edge 1, left
    edge linear 1 -> 0, the other edges 0, a random source of amplitude 1e-3."""
    m = Multigrid2D(MultigridConfig(width=w, height=h, dtype=dtype, **kw), device="cpu")
    m.set_boundary(top=1.0, left=torch.linspace(1.0, 0.0, h, dtype=F64))
    gen = torch.Generator(device="cpu").manual_seed(1)
    m.set_source((2.0 * torch.rand(h, w, generator=gen, dtype=F64) - 1.0) * 1e-3)
    return m


# ------------------------------------------------------------------ the planner
def test_planner_level_lists():
    assert ops.mg_plan_levels(2047, 2047) == [(n, n) for n in (2047, 1023, 511, 255, 127, 63, 31)]
    assert ops.mg_plan_levels(1023, 511) == [(1023, 511), (511, 255), (255, 127), (127, 63), (63, 31), (31, 15)]
    assert ops.mg_plan_levels(35, 67) == [(35, 67), (17, 33), (8, 16)]
    assert ops.mg_plan_levels(8191, 8191)[-1] == (31, 31) and len(ops.mg_plan_levels(8191, 8191)) == 9
    assert ops.mg_plan_levels(6143, 6143)[-1] == (23, 23)
    assert ops.mg_plan_levels(31, 31) == [(31, 31)]
    assert ops.mg_plan_levels(2047, 63)[-1] == (63, 1)


@pytest.mark.parametrize("n", [2048, 2049])
def test_sizes_that_do_not_coarsen_raise_and_name_the_nearest(n):
    with pytest.raises(ValueError, match="2047"):
        ops.mg_plan_levels(n, n)
    with pytest.raises(ValueError, match="does not coarsen"):
        Multigrid2D(MultigridConfig(width=n, height=n), device="cpu")


def test_aspect_ratios_that_end_above_the_coarse_solve_raise():
    with pytest.raises(ValueError, match="127 x 1"):
        ops.mg_plan_levels(2047, 31)


def test_single_level_grids_are_refused():
    with pytest.raises(ValueError, match="single level"):
        Multigrid2D(MultigridConfig(width=31, height=31), device="cpu")


# ------------------------------------------------------------------- the tables
def test_default_smoother_table_is_exactly_the_base_pair():
    t = ops.mg_smoother_table(0.2, 0.2, 0.8, 3)
    assert t == {"n": 3, "center": [0.2] * 3, "neighbor": [0.2] * 3, "weight": [1.0] * 3}
    t = ops.mg_smoother_table(0.0, 0.25, 0.8, 1)
    assert t["weight"] == [0.8] and t["center"] == [1.0 - 0.8] and t["neighbor"] == [0.8 * 0.25]


def test_coarse_plan_reuses_the_leja_ordered_cycle_and_counts_its_repeats():
    p = ops.mg_coarse_plan(31, 15, 0.2, 0.2, 1e-3)
    t = core().chebyshev_cycle(31, 15, 0.2, 0.2, 32)
    assert p["n"] == 32 and p["center"] == list(t["center"]) and p["neighbor"] == list(t["neighbor"])
    assert p["weight"] == [n / 0.2 for n in t["neighbor"]]
    assert 0.0 < p["rho"] < 1.0
    assert p["rho"] ** p["repeats"] <= 1e-3 < p["rho"] ** (p["repeats"] - 1)
    # the bound is the Chebyshev value 1 / T_32 of the spectrum, up to sampling
    a, b = ops.relaxation_spectrum(31, 15, 0.2, 0.2)
    s = (math.sqrt(b / a) - 1) / (math.sqrt(b / a) + 1)
    assert p["rho"] == pytest.approx(2 * s ** 32 / (1 + s ** 64), rel=1e-6)
    assert ops.mg_coarse_plan(31, 15, 0.2, 0.2, 1e-6)["repeats"] > p["repeats"]


@pytest.mark.parametrize("c0,c1", [(0.2, 0.21), (0.5, 0.2), (1.8, -0.2)])
def test_an_operator_that_is_not_the_pure_laplacian_raises(c0, c1):
    with pytest.raises(ValueError, match="pure Laplace"):
        MultigridConfig(width=127, height=127, c_center=c0, c_neighbor=c1)
    with pytest.raises(ValueError, match="pure Laplace"):
        ops.multigrid_vcycle_reference(torch.zeros(129, 129, dtype=F64), torch.zeros(127, 127, dtype=F64), c0, c1)


@pytest.mark.parametrize("kw", [{"nu_pre": 0}, {"nu_post": 5}, {"smoother_omega": 0.0}, {"coarse_reduction": 1.0},
                                {"dtype": "f16"}])
def test_config_errors(kw):
    with pytest.raises(ValueError):
        MultigridConfig(width=127, height=127, **kw)


def test_one_process_only():
    from cuda_mpi_scratch_amd.parallel import DistContext

    with pytest.raises(ValueError, match="one process"):
        Multigrid2D(MultigridConfig(width=127, height=127), DistContext(rank=0, world_size=2), device="cpu")


# -------------------------------------------------------- operators, transfer
@pytest.mark.parametrize("dtype", [F32, F64])
def test_the_sweep_has_the_rounding_points_of_the_per_step_source_reference(dtype):
    gen = torch.Generator(device="cpu").manual_seed(3)
    full = (torch.rand(9, 13, generator=gen, dtype=F64) * 2 - 1).to(dtype)
    g = (torch.rand(7, 11, generator=gen, dtype=F64) * 2 - 1).to(dtype)
    t = core().chebyshev_cycle(11, 7, 0.2, 0.2, 4)
    weight = [n / 0.2 for n in t["neighbor"]]
    got = ops.mg_smooth_reference(full, g, t["center"], t["neighbor"], weight)
    want = ops.jacobi_source_per_step_reference(full, g, t["center"], t["neighbor"], 0.2, hold=15)
    assert torch.equal(got, want)
    assert torch.equal(got[0], full[0]) and torch.equal(got[:, -1], full[:, -1])


def test_prolongation_is_four_times_the_transpose_of_full_weighting():
    """<P e, r> = 4 <e, R r> on 15 x 7 in fp64 (mg_restrict_reference is 4 R)."""
    gen = torch.Generator(device="cpu").manual_seed(5)
    e = torch.rand(3, 7, generator=gen, dtype=F64) * 2 - 1
    r = torch.rand(7, 15, generator=gen, dtype=F64) * 2 - 1
    lhs = float((ops.mg_prolong_reference(e) * r).sum())
    rhs = float((e * ops.mg_restrict_reference(r)).sum())
    assert lhs == pytest.approx(rhs, rel=1e-12, abs=1e-13)


def test_transfer_of_simple_fields():
    # a constant residual restricts to 4 x itself; bilinear P reproduces a linear field away from the edge
    assert torch.equal(ops.mg_restrict_reference(torch.full((7, 15), 0.5, dtype=F64)), torch.full((3, 7), 2.0, dtype=F64))
    e = torch.arange(7, dtype=F64)[None, :].repeat(3, 1)
    p = ops.mg_prolong_reference(e)
    assert p.shape == (7, 15)
    assert torch.equal(p[1:-1, 1:-1], (torch.arange(1, 14, dtype=F64) - 1)[None, :].repeat(5, 1) / 2)
    u = torch.ones(7, 15, dtype=F64)
    assert torch.equal(ops.mg_prolong_add_reference(u, e), u + p)


def test_residual_restrict_reference_matches_the_residual_norm_reference():
    m = prototype(35, 67)
    full = m.full()
    r = ops.mg_residual_reference(full, m._g)
    linf, l2 = ops.residual5_reference(full, 1, 0.2, 0.2, source=m._g)
    assert float(r.abs().max()) == linf and float(torch.sqrt((r * r).sum())) == l2
    assert torch.equal(ops.mg_residual_restrict_reference(full, m._g), ops.mg_restrict_reference(r))


# ---------------------------------------------------------------- convergence
_RUNS = {}


def converge(w, h):
    """The prototype's problem solved to 1e-8 relative l2, once per size."""
    if (w, h) not in _RUNS:
        m = prototype(w, h)
        r0 = m.residual()["l2"]
        _RUNS[(w, h)] = (r0, m.solve(1e-8 * r0, 14))
    return _RUNS[(w, h)]


@pytest.mark.parametrize("w,h", [(127, 127), (511, 255)])
def test_v22_reduces_the_residual_by_five_every_cycle(w, h):
    """Each of the first 6 l2 factors is <= 0.2 (the prototype measured 0.151-0.159)."""
    r0, out = converge(w, h)
    l2 = [c[2] for c in out["history"]]
    factors = [b / a for a, b in zip(l2, l2[1:])][:6]
    print(f"V(2,2) {w}x{h}: factors {[round(f, 4) for f in factors]}, {out['cycles']} cycles, {out['reason']}")
    assert len(factors) == 6 and max(factors) <= 0.2
    assert out["converged"], out["reason"]


def test_cycle_count_does_not_depend_on_the_grid():
    a, b = converge(127, 127)[1], converge(511, 255)[1]
    assert a["converged"] and b["converged"]
    assert abs(a["cycles"] - b["cycles"]) <= 1


def test_fp32_ends_at_its_rounding_floor():
    m = prototype(127, 127, "f32")
    r0 = m.residual()["l2"]
    out = m.solve(0.0, 40)
    print(f"fp32 127x127: {out['reason']} after {out['cycles']} cycles, relative residual {out['residual'] / r0:.3e}")
    assert out["reason"] == "stalled" or out["converged"]
    assert out["residual"] / r0 <= 1e-5
    if out["reason"] == "stalled":  # three cycles without a new best
        best = min(c[2] for c in out["history"])
        assert out["history"][-4][2] == best and all(c[2] >= best for c in out["history"][-3:])


def test_solve_reports_max_cycles_and_non_finite():
    m = prototype(127, 63)
    out = m.solve(0.0, 2)
    assert out["reason"] == "max_cycles reached" and out["cycles"] == 2 and len(out["history"]) == 3
    assert m.cycles_run == 2 and m.sweep_equivalents(2) == pytest.approx(2 * 4 * 4 / 3)
    m.set_field(float("nan"))
    out = m.solve(1e-8, 5)
    assert out["reason"] == "non-finite residual" and out["cycles"] == 0


def test_no_source_and_v13_also_converge():
    m = prototype(35, 67, nu_pre=1, nu_post=3)
    m.set_source(None)
    r0 = m.residual()["l2"]
    out = m.solve(1e-8 * r0, 14)
    assert out["converged"], out
    assert m.levels() == [(35, 67), (17, 33), (8, 16)] and "V(1,3)" in m.note()


def test_manufactured_poisson_solution_within_the_proven_bound():
    """||e||_2 <= ||r||_2 / a for a symmetric A: a theorem, not a measurement."""
    w, h, tol = 127, 63, 1e-10
    u_star, g, a = manufactured(w, h)
    m = Multigrid2D(MultigridConfig(width=w, height=h, dtype="f64"), device="cpu")
    m.set_source(g)
    out = m.solve(tol, 30)
    err = float(torch.linalg.vector_norm(m.field() - u_star))
    print(f"manufactured {w}x{h}: {out['cycles']} cycles, l2 residual {out['residual']:.3e}, ||u - u*||_2 {err:.3e}, "
          f"bound {tol / a:.3e}")
    assert out["converged"], out["reason"]
    assert err <= tol / a
