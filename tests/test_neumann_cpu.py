"""Neumann sides of the CG and PCG Poisson solvers without a GPU: the level
planner with ghost codes (C++ against its Python twin), the coarse interval of
every end-code pair against dense eigenvalues, the property the mirrored
transfers exist for (the V-cycle stays symmetric positive definite), exact
discrete solutions, a dense direct solve, and the iteration counts of the
preconditioned twin against its own all-Dirichlet count."""
import functools
import itertools
import json
import math

import pytest
import torch

from cuda_mpi_scratch_amd import core, ops
from cuda_mpi_scratch_amd.models import cg2d, pcg2d
from cuda_mpi_scratch_amd.models.cg2d import CgConfig, ConjugateGradient2D
from cuda_mpi_scratch_amd.models.pcg2d import MultigridPcg2D, PcgConfig

WEIGHTS = [(0.2, 0.2), (0.5, 0.1)]
ALL = ("top", "bottom", "left", "right")


def level0(w, h, c0, c1, neumann):
    """The finest level's dict, as the planner makes it (a single level for the small grids here)."""
    return ops.pcg_plan_levels_twin(w, h, c0, c1, neumann)[0]


# ------------------------------------------------------------------ 1. the planner
GRIDS = [(2048, 2048), (255, 255), (300, 100), (1000, 333), (513, 64), (20, 17), (1, 1)]
SIDE_SETS = [(("left",), 0.2), (("right", "bottom"), 0.2), (("left", "right", "top"), 0.2), (ALL, 0.19)]


@pytest.mark.parametrize("neumann,c0", SIDE_SETS)
@pytest.mark.parametrize("w,h", GRIDS)
def test_planner_equals_its_python_twin(w, h, neumann, c0):
    native, twin = ops.pcg_plan_levels(w, h, c0, 0.2, neumann), ops.pcg_plan_levels_twin(w, h, c0, 0.2, neumann)
    assert native == twin
    for l in native:
        assert l["reflect_rows"] == (l["bottom"] == -1) and l["reflect_cols"] == (l["right"] == -1)
        assert ops.level_sides(l) == (l["top"], l["bottom"], l["left"], l["right"])
    # Level 0 has the user's sides, near sides inherit the kind on every level.
    assert ops.level_sides(native[0]) == ops.side_codes(neumann)
    assert all((l["top"], l["left"]) == (native[0]["top"], native[0]["left"]) for l in native)
    # Sizes and c0_k do not depend on the sides.
    plain = ops.pcg_plan_levels(w, h, c0, 0.2)
    assert [(l["width"], l["height"], l["c_center"]) for l in native] == \
        [(l["width"], l["height"], l["c_center"]) for l in plain]


def test_planner_far_side_rule_and_errors():
    """300 x 100 with `right` Neumann: right is +1 on every level whatever the
    parity, bottom follows the reflect pattern of the all-Dirichlet plan."""
    for fn in (ops.pcg_plan_levels, ops.pcg_plan_levels_twin):
        lv = fn(300, 100, 0.2, 0.2, ("right",))
        assert [(l["width"], l["height"]) for l in lv] == [(300, 100), (150, 50), (75, 25), (37, 12), (18, 6)]
        assert [l["right"] for l in lv] == [1, 1, 1, 1, 1]
        assert [l["reflect_cols"] for l in lv] == [False] * 5
        assert [l["bottom"] for l in lv] == [0, -1, -1, 0, -1]
        assert [l["reflect_rows"] for l in lv] == [False, True, True, False, True]
        assert all(l["top"] == 0 and l["left"] == 0 for l in lv)
        # Without sides the dicts carry the codes of the flags.
        assert [(l["bottom"], l["right"]) for l in fn(300, 100)] == [(0, 0), (-1, -1), (-1, -1), (0, 0), (-1, 0)]
        with pytest.raises(ValueError, match="singular"):
            fn(64, 64, 0.2, 0.2, ALL)
        with pytest.raises(ValueError, match="unknown side"):
            fn(64, 64, 0.2, 0.2, ("north",))
        fn(64, 64, 0.19, 0.2, ALL)
    for cfg in (CgConfig, PcgConfig):
        with pytest.raises(ValueError, match="Hold one side fixed.*screened"):
            cfg(width=64, height=64, c_center=0.2, c_neighbor=0.2, neumann=ALL)
        with pytest.raises(ValueError, match="unknown side"):
            cfg(width=64, height=64, neumann=("up",))
        with pytest.raises(ValueError, match="twice"):
            cfg(width=64, height=64, neumann=("left", "left"))
        assert cfg(width=64, height=64, neumann=["right", "top"]).neumann == ("top", "right")
        assert cfg(width=64, height=64).neumann == ()
    with pytest.raises(ValueError, match="singular"):
        ops.cg_reference(torch.zeros(6, 6, dtype=torch.float64), torch.ones(4, 4, dtype=torch.float64), neumann=ALL)
    with pytest.raises(ValueError, match="singular"):
        ops.pcg_reference(torch.zeros(6, 6, dtype=torch.float64), torch.ones(4, 4, dtype=torch.float64), neumann=ALL)


# ---------------------------------------------------------- 2. the coarse interval
# The six unordered end-code pairs of an axis as (near, far).
PAIRS = [(0, 0), (1, 0), (1, 1), (0, -1), (1, -1), (-1, -1)]


def dense_level_operator(w, h, c0, c1, sides):
    """L of a level from the reference residual: column i is minus the residual of
    the i-th unit vector with its coded ghosts and no source."""
    n = w * h
    L = torch.zeros(n, n, dtype=torch.float64)
    zero = torch.zeros(h, w, dtype=torch.float64)
    for i in range(n):
        e = torch.zeros((h + 2, w + 2), dtype=torch.float64)
        e[1 + i // w, 1 + i % w] = 1.0
        L[:, i] = -ops.mg_residual_reference(ops.pcg._reflect(e, False, False, sides), zero, c0, c1).reshape(-1)
    return L


def test_axis_mu_closed_forms():
    """The table of docs/ARCHITECTURE.md against eigvalsh of the 1-D neighbour matrix."""
    worst = 0.0
    for n in range(1, 64):
        for s, t in PAIRS:
            N = torch.zeros(n, n, dtype=torch.float64)
            for i in range(n - 1):
                N[i, i + 1] = N[i + 1, i] = 1.0
            N[0, 0] += s
            N[n - 1, n - 1] += t
            mu = float(torch.linalg.eigvalsh(N)[-1])
            level = {"width": n, "height": 1, "reflect_rows": False, "reflect_cols": t == -1, "c_center": 0.0,
                     "top": 1, "bottom": 1, "left": s, "right": t}
            a, _ = ops.pcg_coarse_interval(level, 1.0)  # a = 1 - (mu_x + 2)
            worst = max(worst, abs((1.0 - a - 2.0) - mu))
    print(f"closed forms against eigvalsh, n = 1..63: worst difference {worst:.2e}")
    assert worst <= 1e-13


@pytest.mark.parametrize("w,h", [(16, 16), (7, 12)])
def test_coarse_interval_of_every_end_code_pair(w, h):
    """L == L^T exactly, every eigenvalue in the plan's [a, b], the planned cycle
    contracts; with a mirror side (where the new interval applies) a is the
    smallest eigenvalue to 1e-12. Levels without a mirror side keep the earlier
    interval, whose a is relaxation_spectrum's lower bound and not tight under a
    reflecting side, so tightness is asserted where the closed forms are used.
    All four ends mirrored is singular without screening: that combination runs
    with (0.5, 0.1) only."""
    worst_gap = 0.0
    for (c0, c1), (left, right), (top, bottom) in itertools.product(WEIGHTS, PAIRS, PAIRS):
        sides = (top, bottom, left, right)
        mirror = 1 in sides
        if sides == (1, 1, 1, 1) and c0 == 0.2:
            continue
        level = {"width": w, "height": h, "reflect_rows": bottom == -1, "reflect_cols": right == -1, "c_center": c0,
                 "top": top, "bottom": bottom, "left": left, "right": right}
        L = dense_level_operator(w, h, c0, c1, sides)
        assert float((L - L.T).abs().max()) == 0.0, sides
        ev = torch.linalg.eigvalsh(L)
        a, b = ops.pcg_coarse_interval(level, c1)
        assert a <= float(ev[0]) + 1e-12 and float(ev[-1]) <= b + 1e-12, (sides, a, b, float(ev[0]), float(ev[-1]))
        if mirror:
            worst_gap = max(worst_gap, abs(a - float(ev[0])))
            assert abs(a - float(ev[0])) <= 1e-12, (sides, a, float(ev[0]))
            assert b == 1.0 - c0 + 4.0 * c1
        plan = ops.pcg_coarse_plan(level, c1, 1e-3)
        assert plan["repeats"] >= 1 and plan["rho"] ** plan["repeats"] <= 1e-3, sides
        if mirror:
            assert len(plan["weight"]) == 32
            poly = torch.ones_like(ev)
            for wt in plan["weight"]:
                poly = poly * (1.0 - wt * ev)
            assert float(poly.abs().max()) <= plan["rho"] * (1 + 1e-9), sides
    print(f"{w}x{h}: worst |a - lambda_min| over the mirror levels {worst_gap:.2e}")


def test_nearly_singular_coarse_solve_names_its_cause():
    level = {"width": 16, "height": 16, "reflect_rows": False, "reflect_cols": False, "c_center": 0.2 - 1e-9,
             "top": 1, "bottom": 1, "left": 1, "right": 1}
    with pytest.raises(ValueError, match="nearly singular"):
        ops.pcg_coarse_plan(level, 0.2, 1e-3)


# ------------------------------------------------- 3. the preconditioner as a matrix
def _dense_preconditioner(w, h, c0, c1, neumann):
    plan = ops.PcgPlan(w, h, c0, c1, neumann=neumann)
    n = w * h
    M = torch.zeros(n, n, dtype=torch.float64)
    for i in range(n):
        e = torch.zeros(n, dtype=torch.float64)
        e[i] = 1.0
        M[:, i] = ops.pcg_precondition_reference(e.reshape(h, w), plan).reshape(-1)
    return M, plan


@pytest.mark.parametrize("neumann,c0,c1", [(("left",), 0.2, 0.2), (("right",), 0.2, 0.2), (("top", "bottom"), 0.2, 0.2),
                                           (("left", "bottom"), 0.2, 0.2), (ALL, 0.5, 0.1)])
@pytest.mark.parametrize("w,h", [(33, 40), (40, 33)])
def test_preconditioner_is_symmetric_positive_definite(w, h, neumann, c0, c1):
    """The V-cycle on unit vectors (test_pcg_cpu's bound). Two levels, one axis
    even and one odd, so the doubled restriction rows are exercised on an odd far
    side and left out on an even one: this fails if R is not P^T / 4."""
    M, plan = _dense_preconditioner(w, h, c0, c1, neumann)
    assert len(plan.levels) == 2
    scale = float(M.abs().max())
    asym = float((M - M.T).abs().max())
    ev = torch.linalg.eigvalsh((M + M.T) / 2)
    print(f"{w}x{h} {neumann}: |M - M^T|_max {asym:.3e} of |M|_max {scale:.3e}, eigenvalues {float(ev[0]):.4e} .. "
          f"{float(ev[-1]):.4e}")
    assert asym <= 1e-12 * scale
    assert float(ev[0]) > 0.0


# ------------------------------------------------------ 4. exact discrete solutions
def exact_cases(w, h):
    """(name, config keywords, boundary, source, expected core) of the three exact solutions."""
    s, q = 0.25, 3e-3
    i = torch.arange(h, dtype=torch.float64).reshape(h, 1).expand(h, w)
    j = torch.arange(w, dtype=torch.float64).reshape(1, w).expand(h, w)
    return [
        ("a", dict(neumann=("left", "right")), dict(top=1.0, bottom=0.0), None, 1.0 - (i + 1.0) / (h + 1.0)),
        ("b", dict(neumann=("top", "bottom", "left")), dict(left=-s, right=s * w), None, s * j),
        ("c", dict(neumann=ALL, c_center=0.1, c_neighbor=0.2), dict(), q, torch.full((h, w), q / (1.0 - 0.1 - 0.8),
                                                                                     dtype=torch.float64)),
    ]


@pytest.mark.parametrize("model,config", [(ConjugateGradient2D, CgConfig), (MultigridPcg2D, PcgConfig)])
def test_exact_discrete_solutions(model, config):
    """40 x 24, fp64, l2 <= 1e-11: ||u - u*||_2 <= tol / a with the level-0 a (the
    smallest eigenvalue of L, test_cg_cpu's theorem)."""
    w, h, tol = 40, 24, 1e-11
    for name, kw, boundary, source, expect in exact_cases(w, h):
        cfg = config(width=w, height=h, dtype="f64", **kw)
        m = model(cfg, device="cpu")
        m.set_boundary(**boundary)
        m.set_source(source)
        out = m.solve(tol, 4 * w * h)
        a = ops.pcg_coarse_interval(level0(w, h, cfg.c_center, cfg.c_neighbor, cfg.neumann), cfg.c_neighbor)[0]
        err = float(torch.linalg.vector_norm(m.field() - expect))
        print(f"{model.__name__} ({name}) {cfg.neumann}: {out['iterations']} iterations, residual {out['residual']:.3e}, "
              f"error {err:.3e}, bound {tol / a:.3e}")
        assert out["converged"] and out["residual"] <= tol, out["reason"]
        assert out["residual"] == m.residual()["l2"]
        assert err <= (tol / a) * (1 + 1e-6)
        assert ", ".join(cfg.neumann) in m.note()


# -------------------------------------------------------- 5. the dense direct solve
def neumann_problem(w, h):
    """A random ring (values on Dirichlet sides, differences d on Neumann sides), start and source."""
    gen = torch.Generator(device="cpu").manual_seed(7 * w + h)
    rnd = lambda *s, amp=1.0: (torch.rand(*s, generator=gen, dtype=torch.float64) * 2 - 1) * amp  # noqa: E731
    return {"top": rnd(w), "bottom": rnd(w), "left": rnd(h), "right": rnd(h), "field": rnd(h, w),
            "source": rnd(h, w, amp=1e-2)}


def direct_solution(w, h, c0, c1, prob, neumann):
    full = torch.zeros(h + 2, w + 2, dtype=torch.float64)
    full[0, 1:-1], full[-1, 1:-1] = prob["top"], prob["bottom"]
    full[1:-1, 0], full[1:-1, -1] = prob["left"], prob["right"]
    b = ops.mg_residual_reference(ops.ghosted(full, neumann), prob["source"], c0, c1)
    L = dense_level_operator(w, h, c0, c1, ops.side_codes(neumann))
    return torch.linalg.solve(L, b.reshape(-1)).reshape(h, w)


@pytest.mark.parametrize("model,config", [(ConjugateGradient2D, CgConfig), (MultigridPcg2D, PcgConfig)])
@pytest.mark.parametrize("c0,c1", WEIGHTS)
@pytest.mark.parametrize("neumann", [("left",), ("right", "bottom")])
def test_twin_against_the_dense_direct_solve(neumann, c0, c1, model, config):
    w, h, tol = 40, 24, 1e-11
    prob = neumann_problem(w, h)
    m = model(config(width=w, height=h, dtype="f64", c_center=c0, c_neighbor=c1, neumann=neumann), device="cpu")
    m.set_boundary(top=prob["top"], bottom=prob["bottom"], left=prob["left"], right=prob["right"])
    m.set_field(prob["field"])
    m.set_source(prob["source"])
    out = m.solve(tol, 4 * w * h)
    a = ops.pcg_coarse_interval(level0(w, h, c0, c1, neumann), c1)[0]
    err = float(torch.linalg.vector_norm(m.field() - direct_solution(w, h, c0, c1, prob, neumann)))
    print(f"{model.__name__} {neumann} ({c0}, {c1}): {out['iterations']} iterations, residual {out['residual']:.3e}, "
          f"error {err:.3e}, bound {tol / a:.3e}")
    assert out["converged"] and out["residual"] <= tol, out["reason"]
    assert err <= (tol / a) * (1 + 1e-6)


# ------------------------------------------------------------ 6. iteration counts
@functools.lru_cache(maxsize=None)
def pcg_count(w, h, neumann):
    full = torch.zeros(h + 2, w + 2, dtype=torch.float64)
    g = torch.ones(h, w, dtype=torch.float64)
    out = ops.pcg_reference(full, g, tol=1e-8, max_iters=200, neumann=neumann)
    assert out["converged"], out["reason"]
    return out["iterations"]


@pytest.mark.parametrize("neumann", [("left",), ("left", "right"), ("left", "right", "top")])
@pytest.mark.parametrize("w,h", [(256, 256), (250, 250), (300, 100)])
def test_iteration_counts_against_all_dirichlet(w, h, neumann):
    """f = 1, zero ring, fp64, l2 <= 1e-8: pcg_reference with Neumann sides needs at
    most twice its own all-Dirichlet count (mirrored transfers: <= 1.5x in a model,
    unmirrored ones 3-10x). Measured, all-Dirichlet / {left} / {left, right} /
    {left, right, top}: 256 x 256: 13 / 17 / 17 / 18; 250 x 250: 11 / 14 / 14 /
    14; 300 x 100: 12 / 15 / 15 / 17."""
    base, got = pcg_count(w, h, ()), pcg_count(w, h, neumann)
    print(f"{w}x{h}: all-Dirichlet {base} iterations, Neumann {neumann} {got}")
    assert got <= 2 * base


# --------------------------------------------------------------- the references
def test_references_without_sides_are_todays():
    """The trailing keywords default to none, and none is bit for bit the old call."""
    gen = torch.Generator(device="cpu").manual_seed(99)
    full = torch.rand(9, 12, generator=gen, dtype=torch.float64)
    g = torch.rand(7, 10, generator=gen, dtype=torch.float64)
    r0, r1 = ops.cg_start_reference(full, g, 0.2, 0.2), ops.cg_start_reference(full, g, 0.2, 0.2, neumann=())
    assert torch.equal(r0[0], r1[0]) and r0[1:] == r1[1:]
    # A Neumann side reads edge + ring, once.
    rn = ops.cg_start_reference(full, g, 0.2, 0.2, neumann=("left",))[0]
    moved = full.clone()
    moved[1:-1, 0] = full[1:-1, 1] + full[1:-1, 0]
    assert torch.equal(rn, ops.mg_residual_reference(moved, g, 0.2, 0.2))
    # Apply: the ghost is the edge cell of p_new itself.
    p, q, _ = ops.cg_apply_reference(g, g * 0.5, 0.37, 0.2, 0.2, neumann=ALL)
    z = torch.nn.functional.pad(p[None, None], (1, 1, 1, 1), mode="replicate")[0, 0]
    sums = (z[:-2, 1:-1] + z[2:, 1:-1]) + (z[1:-1, :-2] + z[1:-1, 2:])
    assert torch.equal(q, ops.fma(-0.2, sums.contiguous(), (torch.tensor(0.8, dtype=torch.float64) * p).contiguous()))
    # Five-key level dicts still work everywhere.
    level = {"width": 16, "height": 16, "reflect_rows": True, "reflect_cols": False, "c_center": 0.2}
    assert ops.level_sides(level) == (0, -1, 0, 0)
    e = torch.rand(5, 6, generator=gen, dtype=torch.float64)
    u = torch.rand(11, 13, generator=gen, dtype=torch.float64)
    assert torch.equal(ops.mgp_prolong_add_reference(u, e), ops.mgp_prolong_add_reference(u, e, sides=(0, -1, 0, -1)))
    top = ops.mgp_prolong_add_reference(u, e, sides=(1, 0, 0, 0)) - u
    assert torch.allclose(top[0, 1::2], e[0]) and torch.allclose(top[-1, 1::2], 0.5 * e[-1])


def test_cli_records_the_sides(tmp_path):
    for main, name in ((cg2d.main, "cg"), (pcg2d.main, "pcg")):
        path = tmp_path / f"{name}.jsonl"
        assert main(["--size", "40x24", "--neumann", "left,right", "--device", "cpu", "--json", str(path)]) == 0
        rec = json.loads(path.read_text().splitlines()[-1])
        assert rec["neumann"] == ["left", "right"] and rec["converged"] and math.isfinite(rec["residual"])
        assert rec["config"]["neumann"] == ["left", "right"]
    assert core().PCG_SCALARS_BYTES == 72
