"""Implicit heat steps without a GPU: the theta-scheme coefficients, the
right-hand side against exact rational arithmetic, and the CPU twin of
``ImplicitHeat2D`` against what the scheme is known to do: the amplification of a
sine mode, conservation in an insulated box, the maximum principle of backward
Euler, the l2 stability of Crank-Nicolson, a side that moves in time, the
approach to the steady state, and the model's errors."""
import math
from fractions import Fraction

import pytest
import torch

from cuda_mpi_scratch_amd import core, ops
from cuda_mpi_scratch_amd.models import HeatConfig, ImplicitHeat2D
from cuda_mpi_scratch_amd.models.cg2d import CgConfig, ConjugateGradient2D
from cuda_mpi_scratch_amd.models.pcg2d import MultigridPcg2D, PcgConfig
from cuda_mpi_scratch_amd.parallel import DistContext
from tests.test_one_step_reference_cpu import _round

DT = {"f32": torch.float32, "f64": torch.float64}
EPS64 = 2.0 ** -53  # the unit roundoff of fp64
ALL_SIDES = ("top", "bottom", "left", "right")
NEUMANN_SETS = [tuple(s for k, s in enumerate(ALL_SIDES) if mask >> k & 1) for mask in range(16)]


def _rand(shape, seed, amp=1.0):
    gen = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.rand(*shape, generator=gen, dtype=torch.float64) * 2 - 1) * amp


# ------------------------------------------------------------- coefficients
@pytest.mark.parametrize("theta", [1.0, 0.75, 0.5])
@pytest.mark.parametrize("lam", [0.2, 0.3, 50.0, 1e4])
def test_coefficients(lam, theta):
    h = ops.heat_coefficients(lam, theta)
    assert h == {"lam": lam, "theta": theta, "D": 1.0 + 4.0 * theta * lam, **core().heat_coefficients(lam, theta)}
    F = Fraction
    D = 1 + 4 * F(theta) * F(lam)
    exact = {"c1": F(theta) * F(lam) / D, "a": (1 - 4 * (1 - F(theta)) * F(lam)) / D, "b": (1 - F(theta)) * F(lam) / D,
             "s": 1 / D}
    for k, v in exact.items():  # a handful of fp64 operations each: 4 roundings at the most
        assert abs(F(h[k]) - v) <= 4 * EPS64 * abs(v) + F(2) ** -1070, k
    # the identities, to the rounding of their five terms
    assert abs(h["a"] + 4 * h["b"] - 1 / h["D"]) <= 8 * EPS64
    assert abs(0.0 + 4 * h["c1"] + 1 / h["D"] - 1.0) <= 8 * EPS64
    assert abs(h["s"] - 1 / h["D"]) <= 2 * EPS64 * h["s"]
    assert 0 < h["c1"] < 0.25 and (h["b"] == 0.0) == (theta == 1.0)
    ops.cg_check_sides(0.0, h["c1"], ALL_SIDES)  # screened: legal with four Neumann sides


def test_coefficients_refusals():
    for lam in (0.0, -1.0):
        with pytest.raises(ValueError, match="needs lam = kappa dt / h\\^2 > 0"):
            ops.heat_coefficients(lam, 1.0)
    for lam, theta in [(float("nan"), 1.0), (float("inf"), 1.0), (1.0, float("nan")), (1.0, float("inf"))]:
        with pytest.raises(ValueError, match="must be finite"):
            core().heat_coefficients(lam, theta)
    for theta in (0.49, 0.0, -1.0):
        with pytest.raises(ValueError, match="only conditionally stable.*Stencil2D"):
            ops.heat_coefficients(1.0, theta)
    with pytest.raises(ValueError, match="0.5 <= theta <= 1"):
        ops.heat_coefficients(1.0, 1.01)
    with pytest.raises(ValueError, match="conditionally stable"):
        HeatConfig(width=16, height=16, lam=1.0, theta=0.25)
    with pytest.raises(ValueError, match="lam"):
        HeatConfig(width=16, height=16, lam=0.0)


# ------------------------------------------------- the right-hand side, exactly
def _ring_field(w, h, dtype, seed):
    """Core and ring random in [-1, 1], every ring value non-zero (as a Neumann
    difference too); corners are never read."""
    return _rand((h + 2, w + 2), seed).to(DT[dtype])


def _rational_rhs(full, q, lam, theta, neumann, dtype):
    """Per cell ``(chain, exact, bound)``: the contract's chain evaluated on
    Fractions with every operation rounded once to the element type; the exact
    ``a c + b S + s q`` of the rounded coefficients; and the forward error bound
    of the chain (see test_rhs_is_within_its_roundings_of_the_exact_value)."""
    F = Fraction
    r = lambda x: F(_round(x, dtype))  # noqa: E731
    co = ops.heat_coefficients(lam, theta)
    a, b, s = (r(F(co[k])) for k in ("a", "b", "s"))
    v = full.double().tolist()
    H, W = len(v) - 2, len(v[0]) - 2
    u = F(2) ** -(24 if dtype == "f32" else 53)
    chain, exact, bound = [], [], []
    for y in range(1, H + 1):
        rc, re, rb = [], [], []
        for x in range(1, W + 1):
            c = F(v[y][x])
            raw = {"top": F(v[y - 1][x]), "bottom": F(v[y + 1][x]), "left": F(v[y][x - 1]), "right": F(v[y][x + 1])}
            edge = {"top": y == 1, "bottom": y == H, "left": x == 1, "right": x == W}
            ghost_r, ghost_e, mag = {}, {}, F(0)
            for side, val in raw.items():
                mirror = side in neumann and edge[side]
                ghost_e[side] = c + val if mirror else val
                ghost_r[side] = r(c + val) if mirror else val
                mag += abs(c) + abs(val) if mirror else abs(val)
            S_r = r(r(ghost_r["top"] + ghost_r["bottom"]) + r(ghost_r["left"] + ghost_r["right"]))
            S_e = ghost_e["top"] + ghost_e["bottom"] + ghost_e["left"] + ghost_e["right"]
            g_r = r(b * S_r + r(a * c))  # the fma: one rounding of the exact b S + prod
            g_e = a * c + b * S_e
            # S: every operand passes through 2 additions, 3 with its mirror addition
            k = 3 if any(s_ in neumann and edge[s_] for s_ in raw) else 2
            err = abs(b) * ((1 + u) ** k - 1) * mag + u * abs(a * c) + u * abs(g_r)
            if q is not None:
                qq = F(float(q[y - 1][x - 1]))
                sq = r(s * qq)
                err += u * abs(s * qq)
                g_r = r(g_r + sq)
                err += u * abs(g_r)
                g_e += s * qq
            rc.append(float(g_r))
            re.append(g_e)
            rb.append(err)
        chain.append(rc)
        exact.append(re)
        bound.append(rb)
    return chain, exact, bound


@pytest.mark.parametrize("with_q", [False, True])
@pytest.mark.parametrize("theta", [1.0, 0.5])
@pytest.mark.parametrize("w,h,neumann", [(1, 1, ()), (4, 5, ()), (4, 5, ("top", "right")), (1, 1, ALL_SIDES)]
                         + [(3, 2, n) for n in NEUMANN_SETS])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_rhs_equals_rational_arithmetic(dtype, w, h, neumann, theta, with_q):
    """``heat_rhs_reference`` is the contract's chain, bit for bit, in both types;
    and in fp64 every element is within its roundings of the exact value. The
    bound: S is three additions (four with a mirror ghost: one more on that
    operand), so S_hat = sum of operands times (1 + d)^k, k <= 2 (3 with a
    mirror ghost); the product a c rounds once, the fma once, and with a source
    its product and the last sum once each:
    |g_hat - g| <= |b| ((1 + u)^k - 1) sum |operands| + u |a c| + u |g_hat| (+ u |s q| + u |g_hat'|)."""
    lam = 30.0
    full = _ring_field(w, h, dtype, 100 * w + h)
    q = _rand((h, w), 7 * w + h, 0.5).to(DT[dtype]) if with_q else None
    got = ops.heat_rhs_reference(full, q, lam, theta, neumann)
    assert got.shape == (h, w) and got.dtype == DT[dtype]
    chain, exact, bound = _rational_rhs(full, None if q is None else q.double().tolist(), lam, theta, neumann, dtype)
    want = torch.tensor(chain, dtype=torch.float64).to(DT[dtype])
    assert int((got != want).sum()) == 0
    if dtype == "f64":
        worst = 0.0
        for y in range(h):
            for x in range(w):
                err = abs(Fraction(float(got[y, x])) - exact[y][x])
                assert err <= bound[y][x], (y, x, float(err), float(bound[y][x]))
                worst = max(worst, float(err / bound[y][x]) if bound[y][x] else 0.0)
        print(f"rhs {w}x{h} {neumann} theta {theta} q {with_q}: worst error / bound {worst:.3f}")


def test_start_reference_is_cg_starts_on_the_rounded_g():
    full = _ring_field(9, 6, "f64", 3)
    q = _rand((6, 9), 4)
    for theta in (1.0, 0.5):
        for neumann in ((), ("left", "bottom")):
            g, r, rr, linf = ops.heat_start_reference(full, q, 7.0, theta, neumann)
            c1 = ops.heat_coefficients(7.0, theta)["c1"]
            assert torch.equal(g, ops.heat_rhs_reference(full, q, 7.0, theta, neumann))
            want = ops.cg_start_reference(full, g, 0.0, c1, neumann=neumann)
            assert torch.equal(r, want[0]) and (rr, linf) == want[1:]


# --------------------------------------------------------------- the model
def _model(w, h, lam, theta, method, neumann=(), **kw):
    return ImplicitHeat2D(HeatConfig(width=w, height=h, dtype="f64", lam=lam, theta=theta, method=method,
                                     neumann=neumann, **kw), device="cpu")


def sine_mode(w, h, k, l):
    """``sin(pi k (i + 1) / (H + 1)) sin(pi l (j + 1) / (W + 1))`` and its ``mu``."""
    i = torch.arange(1, h + 1, dtype=torch.float64)
    j = torch.arange(1, w + 1, dtype=torch.float64)
    u0 = torch.outer(torch.sin(math.pi * k * i / (h + 1)), torch.sin(math.pi * l * j / (w + 1)))
    return u0, 4 - 2 * math.cos(math.pi * k / (h + 1)) - 2 * math.cos(math.pi * l / (w + 1))


def amplification_check(make, w, h, lam, theta, n=5, mode=(2, 3)):
    """``||u_n - rho^n u0||_2 <= n D tol (1 + 1e-6) + 64 eps64 ||u0||_2``: every step
    is off by at most D tol and the step map is a contraction in l2 (|rho| <= 1
    for every mode), so the solve errors add up; the second term covers the
    rounding of the n right-hand sides and of the sine table."""
    u0, mu = sine_mode(w, h, *mode)
    rho = (1 - (1 - theta) * lam * mu) / (1 + theta * lam * mu)
    assert abs(rho) <= 1
    norm0 = float(torch.linalg.vector_norm(u0))
    tol = 1e-12 * norm0
    m = make()
    m.set_field(u0)
    out = m.step(n, tol)
    assert out["converged"] and out["steps"] == n, out
    err = float(torch.linalg.vector_norm(m.field().cpu() - rho ** n * u0))
    D = 1 + 4 * theta * lam
    bound = n * D * tol * (1 + 1e-6) + 64 * EPS64 * norm0
    print(f"amplification {w}x{h} lam {lam} theta {theta} {m.cfg.method}: rho {rho:.6f}, iterations {out['iterations']}, "
          f"||u_n - rho^n u0||_2 {err:.3e}, bound {bound:.3e}")
    assert err <= bound


@pytest.mark.parametrize("method", ["pcg", "cg"])
@pytest.mark.parametrize("lam", [0.2, 50.0, 1e4])
@pytest.mark.parametrize("theta", [1.0, 0.5])
def test_amplification_of_a_sine_mode(theta, lam, method):
    amplification_check(lambda: _model(33, 21, lam, theta, method), 33, 21, lam, theta)


@pytest.mark.parametrize("method", ["pcg", "cg"])
@pytest.mark.parametrize("theta", [1.0, 0.5])
def test_an_insulated_box_conserves_heat(theta, method):
    """Four Neumann sides with zero flux. In exact arithmetic sum(g) = (a + 4 b)
    sum(u) = sum(u) / D and every row sum of L is 1 / D, so sum(u') = sum(u); a
    residual r moves the sum by D sum(r), |sum(r)| <= sqrt(N) ||r||_2 <= sqrt(N) tol.
    Rounding: the right-hand side and the evaluation of the residual that meets
    tol are off per cell by at most 4 u (|c| + |n| + |s| + |w| + |e|) together (the
    chains of test_rhs_equals_rational_arithmetic with |a| < 1, b, c1 < 1/4), a
    cell is an operand of at most 5 cells, and the sum of these per-cell errors
    is amplified by D as well: D 20 u sum |u| per step. The sums here are exact
    (math.fsum)."""
    w, h, lam, n, tol = 20, 12, 30.0, 4, 1e-10
    N, D = w * h, 1 + 4 * theta * lam
    m = _model(w, h, lam, theta, method, neumann=ALL_SIDES)
    m.set_field(_rand((h, w), 17) + 0.5)
    total0 = math.fsum(m.field().reshape(-1).tolist())
    slack = 0.0
    for k in range(n):
        slack += D * math.sqrt(N) * tol + D * 20 * EPS64 * math.fsum(abs(v) for v in m.field().reshape(-1).tolist())
        out = m.step(1, tol)
        assert out["converged"], out
        drift = abs(math.fsum(m.field().reshape(-1).tolist()) - total0)
        print(f"insulated {method} theta {theta} step {k + 1}: {out['iterations']} iterations, |sum(u) - sum(u0)| "
              f"{drift:.3e}, bound {slack:.3e}")
        assert drift <= slack
    assert out["time_steps_total"] == n


@pytest.mark.parametrize("method", ["pcg", "cg"])
def test_backward_euler_keeps_the_maximum_principle_at_a_stiff_step(method):
    """L is an M-matrix whose rows (with the ring's weights) sum to 1 - 1/D, and g =
    u / D >= 0: the exact step of data in [0, 1] stays in [0, 1], a field in [-d, 1 +
    d] in [-d, 1 + d]. A step solved to tol is off by at most D tol in l2, hence in
    every cell: after k steps every value is in [-k D tol, 1 + k D tol]."""
    w = h = 24
    lam, tol = 1e4, 1e-9
    D = 1 + 4 * lam
    m = _model(w, h, lam, 1.0, method)
    m.set_boundary(top=(_rand((w,), 1) + 1) / 2, bottom=1.0, left=0.0, right=(_rand((h,), 2) + 1) / 2)
    m.set_field((_rand((h, w), 3) + 1) / 2)
    for k in (1, 2, 3):
        out = m.step(1, tol)
        u = m.field()
        lo, hi = float(u.min()), float(u.max())
        print(f"maximum principle {method} step {k}: {out['iterations']} iterations, min {lo:.3e}, max - 1 {hi - 1:.3e}, "
              f"D tol {D * tol:.3e}")
        assert out["converged"] and -k * D * tol <= lo and hi <= 1 + k * D * tol


@pytest.mark.parametrize("method", ["pcg", "cg"])
def test_crank_nicolson_stays_bounded_at_a_stiff_step(method):
    """With zero sides every mode is multiplied by |rho| <= 1: ||u_n||_2 <= ||u_0||_2 + n D tol."""
    w = h = 24
    lam, tol, n = 1e4, 1e-9, 4
    D = 1 + 4 * 0.5 * lam
    m = _model(w, h, lam, 0.5, method)
    u0 = (_rand((h, w), 3) + 1) / 2
    m.set_field(u0)
    out = m.step(n, tol)
    have, start = float(torch.linalg.vector_norm(m.field())), float(torch.linalg.vector_norm(u0))
    print(f"Crank-Nicolson {method} lam {lam}: ||u_n||_2 {have:.6f}, ||u_0||_2 {start:.6f}, iterations {out['iterations']}")
    assert out["converged"] and have <= start + n * D * tol


def test_a_side_that_moves_in_time():
    """The ring is read as it stands at each step: a step after set_boundary differs
    from the step without it, and equals the twin's step on the changed ring."""
    w, h, lam = 12, 9, 5.0
    a, b = _model(w, h, lam, 0.5, "cg"), _model(w, h, lam, 0.5, "cg")
    for m in (a, b):
        m.set_boundary(top=1.0, left=0.5)
        m.set_field(_rand((h, w), 5))
        m.step(1, 1e-11)
    assert torch.equal(a.full(), b.full())
    b.set_boundary(top=2.0)
    before = b.full()
    a.step(1, 1e-11)
    b.step(1, 1e-11)
    assert float((a.field() - b.field()).abs().max()) > 1e-3
    want = ops.heat_step_reference(before, None, lam, 0.5, 1e-11, 10000, "l2", "cg")
    assert torch.equal(b.full(), want["full"]) and bool((b.full()[0, 1:-1] == 2.0).all())


@pytest.mark.parametrize("method", ["pcg", "cg"])
def test_a_constant_source_approaches_the_steady_state(method):
    """With q = dt f the fixed point of the step is lam (S - 4 u) + q = 0: the
    solution of u = S / 4 + q / (4 lam), the project's Poisson problem with weights
    (0, 1/4). The error is multiplied per step by the step map, whose l2 norm is
    rho_max = max |rho(mu)| (backward Euler: 1 / (1 + lam mu_min)), and every solve
    adds at most D tol: ||u_n - u_inf||_2 <= rho_max^n ||u_0 - u_inf||_2 + n D tol +
    tol_s / a_s, the last term the steady solve's own error."""
    w, h, lam, n, tol, q = 15, 11, 20.0, 8, 1e-11, 0.3
    D = 1 + 4 * lam
    if method == "pcg":
        s = MultigridPcg2D(PcgConfig(width=w, height=h, dtype="f64", c_center=0.0, c_neighbor=0.25), device="cpu")
    else:
        s = ConjugateGradient2D(CgConfig(width=w, height=h, dtype="f64", c_center=0.0, c_neighbor=0.25), device="cpu")
    s.set_source(q / (4 * lam))
    tol_s = 1e-13
    assert s.solve(tol_s, 2000)["converged"]
    u_inf, a_s = s.field(), ops.relaxation_spectrum(w, h, 0.0, 0.25)[0]
    mu_min = 4 - 2 * math.cos(math.pi / (h + 1)) - 2 * math.cos(math.pi / (w + 1))
    rho_max = 1 / (1 + lam * mu_min)
    m = _model(w, h, lam, 1.0, method)
    m.set_source(q)
    e0 = float(torch.linalg.vector_norm(u_inf))  # the start is u = 0
    for k in range(1, n + 1):
        out = m.step(1, tol)
        assert out["converged"], out
        err = float(torch.linalg.vector_norm(m.field() - u_inf))
        bound = rho_max ** k * e0 + k * D * tol + tol_s / a_s
        print(f"steady state {method} step {k}: error {err:.3e}, bound {bound:.3e} (rho_max {rho_max:.4f})")
        assert err <= bound * (1 + 1e-6)
    assert err <= 1e-3 * e0


def test_model_errors_and_notes():
    with pytest.raises(ValueError, match="one process"):
        ImplicitHeat2D(HeatConfig(width=16, height=16), DistContext(rank=0, world_size=2), device="cpu")
    with pytest.raises(ValueError, match="too thin to coarsen.*ConjugateGradient2D"):
        HeatConfig(width=3000, height=4, lam=2.0, method="pcg")
    HeatConfig(width=3000, height=4, lam=2.0, method="cg")
    with pytest.raises(ValueError, match="method must be"):
        HeatConfig(width=16, height=16, method="auto")
    with pytest.raises(ValueError, match="unknown side"):
        HeatConfig(width=16, height=16, neumann=("north",))
    with pytest.raises(ValueError, match="dtype"):
        HeatConfig(width=16, height=16, dtype="f16")
    m = _model(16, 12, 3.0, 0.5, "pcg", neumann=("left",))
    with pytest.raises(ValueError, match="shape"):
        m.set_source(torch.zeros(16, 12))
    with pytest.raises(ValueError, match="shape"):
        m.set_field(torch.zeros(16, 12))
    with pytest.raises(ValueError, match="norm"):
        m.step(1, 1e-8, norm="l1")
    with pytest.raises(ValueError, match="check_every"):
        m.step(1, 1e-8, check_every=0)
    with pytest.raises(ValueError, match="tol >= 0"):
        m.step(1, -1.0)
    note = m.note()
    for part in ("lam 3", "theta 0.5", "D = 1 + 4 theta lam = 7", f"c1 {m.coeffs['c1']:.17g}", "method pcg",
                 "error per step <= D tol in l2", "Crank-Nicolson", "Neumann sides left"):
        assert part in note, (part, note)
    assert m.step(0, 1e-8) == {"steps": 0, "converged": True, "iterations": [], "residuals": [], "restarts": [],
                               "reason": "", "time_steps_total": 0}


def test_a_step_that_does_not_converge_is_reported():
    m = _model(33, 21, 50.0, 1.0, "cg")
    m.set_field(_rand((21, 33), 8))
    out = m.step(3, 1e-12, max_iters=2)
    assert not out["converged"] and out["steps"] == 0 and out["reason"] == "max_iters reached"
    assert out["iterations"] == [2] and len(out["residuals"]) == 1 and out["residuals"][0] > 1e-12
    assert out["time_steps_total"] == 0 and m.unfinished == "max_iters reached"
    assert out["residuals"][0] == m.residual()["l2"]  # g is the unfinished step's right-hand side
    with pytest.raises(RuntimeError, match="did not converge \\(max_iters reached\\).*set_field"):
        m.step(1, 1e-12)
    m.set_field(_rand((21, 33), 8))
    out = m.step(2, 1e-10)
    assert out["converged"] and out["steps"] == 2 and out["time_steps_total"] == 2
    assert out["residuals"][-1] == m.residual()["l2"] <= 1e-10
