"""Multigrid-preconditioned CG without a GPU: the any-size level planner (C++
against its Python twin), the property everything rests on (the V-cycle is a
symmetric positive-definite operator), the coarse solve's interval on a
reflecting level, the pure-torch twin against a dense direct solve, iteration
counts against plain CG, bit equality with today's cycle where both apply, and
the CPU model's surface."""
import math

import pytest
import torch

from cuda_mpi_scratch_amd import core, ops
from cuda_mpi_scratch_amd.models.pcg2d import MultigridPcg2D, PcgConfig
from tests.test_cg_cpu import direct_solution, ring_problem, setup

WEIGHTS = [(0.2, 0.2), (0.5, 0.1)]


def _sizes(levels):
    return [(l["width"], l["height"]) for l in levels]


# ------------------------------------------------------------------ the planner
@pytest.mark.parametrize("w,h,c0,c1", [(2048, 2048, 0.2, 0.2), (255, 255, 0.2, 0.2), (3000, 1000, 0.2, 0.2),
                                       (1024, 40, 0.2, 0.2), (20, 17, 0.2, 0.2), (250, 250, 0.5, 0.1),
                                       (512, 300, 0.1999, 0.2), (100, 37, 0.2, 0.2), (1, 1, 0.2, 0.2)])
def test_planner_equals_its_python_twin(w, h, c0, c1):
    assert ops.pcg_plan_levels(w, h, c0, c1) == ops.pcg_plan_levels_twin(w, h, c0, c1)


def test_planner_cases():
    lv = ops.pcg_plan_levels(2048, 2048)
    assert len(lv) == 8 and _sizes(lv)[-1] == (16, 16) and _sizes(lv)[1] == (1024, 1024)
    assert not lv[0]["reflect_rows"] and not lv[0]["reflect_cols"]
    assert all(l["reflect_rows"] and l["reflect_cols"] for l in lv[1:])
    # An odd x odd grid is today's multigrid plan, with no flags.
    lv = ops.pcg_plan_levels(255, 255)
    assert _sizes(lv) == [tuple(s) for s in ops.mg_plan_levels(255, 255)]
    assert not any(l["reflect_rows"] or l["reflect_cols"] for l in lv)
    assert all(l["c_center"] == 0.2 for l in lv)
    assert _sizes(ops.pcg_plan_levels(3000, 1000))[-1] == (23, 7)
    assert _sizes(ops.pcg_plan_levels(1024, 40))[-1] == (32, 1)
    assert _sizes(ops.pcg_plan_levels(20, 17)) == [(20, 17)]
    # Flags per axis: 300 x 100 -> 150 x 50 (both even) -> 75 x 25 -> 37 x 12 (odd parents).
    lv = ops.pcg_plan_levels(300, 100)
    assert _sizes(lv) == [(300, 100), (150, 50), (75, 25), (37, 12), (18, 6)]
    assert [(l["reflect_cols"], l["reflect_rows"]) for l in lv] == [(False, False), (True, True), (True, True),
                                                                    (False, False), (False, True)]
    for fn in (ops.pcg_plan_levels, ops.pcg_plan_levels_twin):
        with pytest.raises(ValueError, match="ConjugateGradient2D"):
            fn(3000, 4)
        with pytest.raises(ValueError):
            fn(0, 4)
        with pytest.raises(ValueError):
            fn(64, 64, 0.3, 0.2)


def test_screened_levels():
    """c0_k = 1 - 4 c1 - 4^k sigma, sigma = 1 - c0 - 4 c1 (here 1e-4)."""
    c0, c1 = 0.1999, 0.2
    sigma = 1.0 - c0 - 4.0 * c1
    lv = ops.pcg_plan_levels(512, 300, c0, c1)
    assert lv[0]["c_center"] == c0
    for k, l in enumerate(lv):
        assert l["c_center"] == pytest.approx(1.0 - 4.0 * c1 - 4.0 ** k * sigma, abs=1e-14)
        assert 1.0 - l["c_center"] - 4.0 * c1 >= 0.0  # still admissible: the level's own sigma
    assert lv[-1]["c_center"] < lv[0]["c_center"]


# -------------------------------------------------- the preconditioner as a matrix
def _dense_preconditioner(w, h, c0, c1):
    plan = ops.PcgPlan(w, h, c0, c1)
    n = w * h
    M = torch.zeros(n, n, dtype=torch.float64)
    for i in range(n):
        e = torch.zeros(n, dtype=torch.float64)
        e[i] = 1.0
        M[:, i] = ops.pcg_precondition_reference(e.reshape(h, w), plan).reshape(-1)
    return M, plan


@pytest.mark.parametrize("c0,c1", WEIGHTS)
@pytest.mark.parametrize("w,h", [(12, 10), (16, 16), (33, 40)])
def test_preconditioner_is_symmetric_positive_definite(w, h, c0, c1):
    """The V-cycle applied to unit vectors: symmetric to rounding (every entry is
    a sum of O(100) products of magnitude <= |M|, each rounded at 2^-53), and
    all eigenvalues positive. (12, 10) and (16, 16) are single levels (the
    coarse solve alone); (33, 40) has a reflecting coarse level on one axis."""
    M, plan = _dense_preconditioner(w, h, c0, c1)
    scale = float(M.abs().max())
    asym = float((M - M.T).abs().max())
    ev = torch.linalg.eigvalsh((M + M.T) / 2)
    print(f"{w}x{h} ({c0}, {c1}): {len(plan.levels)} levels, |M - M^T|_max {asym:.3e} of |M|_max {scale:.3e}, "
          f"eigenvalues {float(ev[0]):.4e} .. {float(ev[-1]):.4e}")
    assert asym <= 1e-12 * scale
    assert float(ev[0]) > 0.0


def test_coarse_interval_of_a_reflecting_level():
    """A reflecting 16 x 16 level: its dense operator's spectrum lies inside the
    interval the plan uses and NOT inside relaxation_spectrum's, whose upper end
    1 - c0 + 4 c1 mu the diagonal shift + c1 exceeds. The cycle built on the
    plan's interval contracts on every eigenvalue."""
    w = h = 16
    c0, c1 = 0.2, 0.2
    level = {"width": w, "height": h, "reflect_rows": True, "reflect_cols": True, "c_center": c0}
    n = w * h
    L = torch.zeros(n, n, dtype=torch.float64)
    for i in range(n):
        e = torch.zeros((h + 2, w + 2), dtype=torch.float64)
        e[1 + i // w, 1 + i % w] = 1.0
        e = ops.pcg._reflect(e, True, True)
        # L v = v - A v: minus the residual of v with no source.
        L[:, i] = -ops.mg_residual_reference(e, torch.zeros(h, w, dtype=torch.float64), c0, c1).reshape(-1)
    assert float((L - L.T).abs().max()) == 0.0
    ev = torch.linalg.eigvalsh(L)
    a, b = ops.pcg_coarse_interval(level, c1)
    a0, b0 = ops.relaxation_spectrum(w, h, c0, c1)
    print(f"eigenvalues {float(ev[0]):.6f} .. {float(ev[-1]):.6f}; plan [{a:.6f}, {b:.6f}]; "
          f"relaxation_spectrum [{a0:.6f}, {b0:.6f}]")
    assert a == a0 and b == 1.0 - c0 + 4.0 * c1
    assert a <= float(ev[0]) and float(ev[-1]) <= b
    assert float(ev[-1]) > b0
    plan = ops.pcg_coarse_plan(level, c1, 1e-3)
    assert plan["repeats"] >= 1 and plan["rho"] ** plan["repeats"] <= 1e-3
    poly = torch.ones_like(ev)
    for wt in plan["weight"]:
        poly = poly * (1.0 - wt * ev)
    assert float(poly.abs().max()) <= plan["rho"] * (1 + 1e-9)
    # Without flags the plan is mg_coarse_plan, double for double.
    flat = dict(level, reflect_rows=False, reflect_cols=False)
    assert ops.pcg_coarse_plan(flat, c1, 1e-3) == ops.mg_coarse_plan(w, h, c0, c1, 1e-3)
    # On relaxation_spectrum's own interval the new function gives chebyshev_cycle's table.
    t0, t1 = ops.chebyshev_cycle(w, h, c0, c1, 32), ops.chebyshev_cycle_interval(a0, b0, c0, c1, 32)
    assert t0["center"] == t1["center"] and t0["neighbor"] == t1["neighbor"]


# --------------------------------------------------------------------- the twin
@pytest.mark.parametrize("c0,c1", WEIGHTS)
def test_twin_against_the_dense_direct_solve(c0, c1):
    """40 x 24 with a non-zero ring and source: ||u - u_direct||_2 <= ||r||_2 /
    lambda_min(L) <= tol / a (test_cg_cpu's theorem)."""
    w, h, tol = 40, 24, 1e-10
    prob = ring_problem(w, h)
    m = MultigridPcg2D(PcgConfig(width=w, height=h, dtype="f64", c_center=c0, c_neighbor=c1), device="cpu")
    setup(m, prob)
    out = m.solve(tol, 200)
    a = ops.relaxation_spectrum(w, h, c0, c1)[0]
    err = float(torch.linalg.vector_norm(m.field() - direct_solution(w, h, c0, c1, prob)))
    print(f"pcg twin {w}x{h} ({c0}, {c1}): {out['iterations']} iterations, true l2 residual {out['residual']:.3e}, "
          f"||u - u_direct||_2 {err:.3e}, bound {tol / a:.3e}")
    assert out["converged"] and out["residual"] <= tol, out["reason"]
    assert out["residual"] == m.residual()["l2"]
    assert err <= (tol / a) * (1 + 1e-6)
    assert out["iterations"] <= 20


@pytest.mark.parametrize("w,h", [(256, 256), (250, 250), (300, 100)])
def test_iteration_counts_against_plain_cg(w, h):
    """f = 1, zero ring, fp64, l2 <= 1e-8. Measured on the CPU twins (iterations
    of pcg_reference / cg_reference): 256 x 256: 13 / 544; 250 x 250: 11 / 531;
    300 x 100: 12 / 463. The bound (one fifth of plain CG) is a guard."""
    full = torch.zeros(h + 2, w + 2, dtype=torch.float64)
    g = torch.ones(h, w, dtype=torch.float64)
    pcg = ops.pcg_reference(full, g, tol=1e-8, max_iters=100)
    cg = ops.cg_reference(full, g, tol=1e-8, max_iters=5000)
    print(f"{w}x{h}: pcg {pcg['iterations']} iterations, cg {cg['iterations']}")
    assert pcg["converged"] and cg["converged"]
    assert 5 * pcg["iterations"] <= cg["iterations"]


def test_equals_todays_cycle_where_both_apply():
    """127 x 63, pure Laplace weights: one preconditioner application is one
    multigrid_vcycle_reference cycle from a zero field with ring 0 and g = r."""
    w, h = 127, 63
    gen = torch.Generator(device="cpu").manual_seed(12763)
    for dtype in (torch.float64, torch.float32):
        r = (torch.rand(h, w, generator=gen, dtype=torch.float64) * 2 - 1).to(dtype)
        z = ops.pcg_precondition_reference(r, ops.PcgPlan(w, h))
        ref = ops.multigrid_vcycle_reference(torch.zeros(h + 2, w + 2, dtype=dtype), r)[1:-1, 1:-1]
        assert z.dtype == dtype and torch.equal(z, ref)


# -------------------------------------------------------------------- the model
def test_model_surface_and_errors():
    with pytest.raises(ValueError, match="nu_pre must equal nu_post"):
        PcgConfig(width=64, height=64, nu_pre=2, nu_post=1)
    with pytest.raises(ValueError, match="ConjugateGradient2D"):
        PcgConfig(width=3000, height=4)
    with pytest.raises(ValueError):
        PcgConfig(width=64, height=64, c_center=0.3, c_neighbor=0.2)
    with pytest.raises(ValueError):
        PcgConfig(width=64, height=64, dtype="f16")
    with pytest.raises(ValueError):
        PcgConfig(width=64, height=64, nu_pre=5, nu_post=5)
    m = MultigridPcg2D(PcgConfig(width=50, height=36, dtype="f32"), device="cpu")
    assert "torch references" in m.note() and "2 levels" in m.note()
    m.set_boundary(top=1.0)
    m.set_source(1e-3)
    with pytest.raises(ValueError):
        m.solve(1e-3, norm="l1")
    out = m.solve(1e-5, 50, "linf")
    assert out["reason"] in ("converged: linf residual <= tol", "stalled") and math.isfinite(out["residual"])
    assert out["iterations"] == m.iterations_run and out["history"][0][0] == 0
    assert torch.isfinite(m.field()).all()
    with pytest.raises(RuntimeError):
        m.scalars()
    # max_iters is honoured, and a converged start costs no iteration.
    m2 = MultigridPcg2D(PcgConfig(width=50, height=36), device="cpu")
    m2.set_source(1.0)
    out = m2.solve(1e-12, 2)
    assert out["iterations"] == 2 and out["reason"] == "max_iters reached" and not out["converged"]
    out = m2.solve(1e30, 5)
    assert out["iterations"] == 0 and out["converged"]
    assert core().PCG_SCALARS_BYTES == 72
