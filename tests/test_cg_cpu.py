"""Conjugate gradients without a GPU: the operator check, the pure-torch twin
against a dense direct solve, the one-iteration eigenvector case, the
L-conjugacy of successive directions, and the CPU model's surface."""
import math

import pytest
import torch

from cuda_mpi_scratch_amd import core, ops
from cuda_mpi_scratch_amd.models.cg2d import CgConfig, ConjugateGradient2D
from tests.test_source_cpu import manufactured

WEIGHTS = [(0.2, 0.2), (0.5, 0.1)]


def test_operator_check():
    for c0, c1 in [(0.2, 0.2), (0.5, 0.1), (0.6, 0.1)]:
        core().cg_check_operator(c0, c1)
        ops.cg_check_operator(c0, c1)
    for c0, c1 in [(0.2, 0.0), (0.2, -0.2), (0.3, 0.2), (0.61, 0.1), (1.0, 0.25)]:
        with pytest.raises(ValueError, match="c_neighbor > 0 and c_center \\+ 4 c_neighbor <= 1"):
            core().cg_check_operator(c0, c1)
    with pytest.raises(ValueError):
        CgConfig(width=8, height=8, c_center=0.3, c_neighbor=0.2)


def dense_operator(w, h, c0, c1):
    """L = (1 - c0) I - c1 (the four neighbours inside the core), row-major cells."""
    n = w * h
    L = torch.zeros(n, n, dtype=torch.float64)
    for y in range(h):
        for x in range(w):
            i = y * w + x
            L[i, i] = 1.0 - c0
            for dx, dy in ((1, 0), (-1, 0), (0, 1), (0, -1)):
                if 0 <= x + dx < w and 0 <= y + dy < h:
                    L[i, (y + dy) * w + (x + dx)] = -c1
    return L


def ring_problem(w, h):
    """A non-zero ring on all sides, a random start and a random source (fp64, CPU)."""
    gen = torch.Generator(device="cpu").manual_seed(5 * w + h)
    rnd = lambda *s, amp=1.0: (torch.rand(*s, generator=gen, dtype=torch.float64) * 2 - 1) * amp  # noqa: E731
    return {"top": 1.0, "bottom": rnd(w), "left": torch.linspace(1.0, 0.0, h, dtype=torch.float64), "right": -0.5,
            "field": rnd(h, w), "source": rnd(h, w, amp=1e-2)}


def direct_solution(w, h, c0, c1, prob):
    """u with L u = b: b is the residual (A u + g) - u of the zero core inside the ring."""
    full = torch.zeros(h + 2, w + 2, dtype=torch.float64)
    full[0, 1:-1], full[-1, 1:-1] = prob["top"], prob["bottom"]
    full[1:-1, 0], full[1:-1, -1] = prob["left"], prob["right"]
    b = ops.mg_residual_reference(full, prob["source"], c0, c1)
    return torch.linalg.solve(dense_operator(w, h, c0, c1), b.reshape(-1)).reshape(h, w)


def setup(m, prob):
    m.set_boundary(top=prob["top"], bottom=prob["bottom"], left=prob["left"], right=prob["right"])
    m.set_field(prob["field"])
    m.set_source(prob["source"])


@pytest.mark.parametrize("c0,c1", WEIGHTS)
@pytest.mark.parametrize("w,h", [(35, 19), (16, 8)])
def test_twin_against_the_dense_direct_solve(w, h, c0, c1):
    """||u - u_direct||_2 <= ||r||_2 / lambda_min(L) <= tol / a, a theorem for a
    symmetric positive definite L; a is the lower end of relaxation_spectrum."""
    tol = 1e-10
    prob = ring_problem(w, h)
    m = ConjugateGradient2D(CgConfig(width=w, height=h, dtype="f64", c_center=c0, c_neighbor=c1), device="cpu")
    setup(m, prob)
    out = m.solve(tol, 4 * w * h)
    a = ops.relaxation_spectrum(w, h, c0, c1)[0]
    err = float(torch.linalg.vector_norm(m.field() - direct_solution(w, h, c0, c1, prob)))
    print(f"twin {w}x{h} ({c0}, {c1}): {out['iterations']} iterations, {out['restarts']} restarts, true l2 residual "
          f"{out['residual']:.3e}, ||u - u_direct||_2 {err:.3e}, bound {tol / a:.3e}")
    assert out["converged"] and out["residual"] <= tol, out["reason"]
    assert out["residual"] == m.residual()["l2"]
    assert err <= (tol / a) * (1 + 1e-6)


def test_an_eigenvector_source_converges_in_one_iteration():
    w, h = 96, 64
    u_star, g, a = manufactured(w, h)
    m = ConjugateGradient2D(CgConfig(width=w, height=h, dtype="f64"), device="cpu")
    m.set_source(g)
    out = m.solve(1e-12, 50)
    err = float(torch.linalg.vector_norm(m.field() - u_star))
    print(f"eigenvector source {w}x{h}: {out['iterations']} iteration(s), residual {out['residual']:.3e}, error {err:.3e}")
    assert out["converged"] and out["iterations"] == 1
    assert err <= (1e-12 / a) * (1 + 1e-6)


@pytest.mark.parametrize("c0,c1", WEIGHTS)
def test_successive_directions_are_conjugate(c0, c1):
    """p_k . L p_{k+1} = 0 in exact arithmetic. In floating point the local
    conjugacy of CG is lost at the rate of the rounding unit times the condition
    number kappa = b / a of L per step (each of beta, p and q carries a few
    relative roundings, amplified by at most kappa in the L-inner product), so the
    bound is 100 kappa 2^-53 relative to ||p_k|| ||L p_{k+1}||, with 100 for the
    handful of operations per step and the sum over the 665 cells. A lost
    orthogonality is of order 1."""
    w, h = 35, 19
    prob = ring_problem(w, h)
    full = torch.zeros(h + 2, w + 2, dtype=torch.float64)
    full[0, 1:-1], full[-1, 1:-1] = prob["top"], prob["bottom"]
    full[1:-1, 0], full[1:-1, -1] = prob["left"], prob["right"]
    full[1:-1, 1:-1] = prob["field"]
    dirs = []
    out = ops.cg_reference(full, prob["source"], c0, c1, 1e-10, 30, on_iteration=lambda k, p, q: dirs.append((k, p, q)))
    assert out["iterations"] == 30 and [k for k, _, _ in dirs] == list(range(30))
    worst = 0.0
    for (_, p0, _), (_, p1, q1) in zip(dirs, dirs[1:]):
        rel = abs(float((p0 * q1).sum())) / (float(torch.linalg.vector_norm(p0)) * float(torch.linalg.vector_norm(q1)))
        worst = max(worst, rel)
    a, b = ops.relaxation_spectrum(w, h, c0, c1)
    bound = 100 * (b / a) * 2.0 ** -53
    print(f"conjugacy ({c0}, {c1}): worst |p_k . L p_k+1| / (||p_k|| ||L p_k+1||) = {worst:.3e}, bound {bound:.3e}")
    assert worst <= bound
    # q is L p: against the dense operator
    L = dense_operator(w, h, c0, c1)
    _, p, q = dirs[7]
    assert torch.allclose((L @ p.reshape(-1)).reshape(h, w), q, rtol=0, atol=1e-14 * float(p.abs().max()) * 8)


def test_step_references_fix_the_scalars():
    """One iteration by hand: alpha = rr / pq, beta = rr' / rr, in double."""
    w, h = 16, 8
    prob = ring_problem(w, h)
    full = torch.zeros(h + 2, w + 2, dtype=torch.float32)
    full[1:-1, 1:-1] = prob["field"].float()
    r, rr, linf = ops.cg_start_reference(full, prob["source"].float(), 0.5, 0.1)
    assert r.dtype == torch.float32 and rr == float((r.double() ** 2).sum()) and linf == float(r.abs().max())
    p, q, pq = ops.cg_apply_reference(r, r, 0.0, 0.5, 0.1)
    assert torch.equal(p, r) and pq > 0
    u1, r1, rr1, _ = ops.cg_update_reference(full[1:-1, 1:-1], r, p, q, rr / pq)
    assert rr1 < rr and u1.dtype == torch.float32
    out = ops.cg_reference(full, prob["source"].float(), 0.5, 0.1, 0.0, 1)
    assert out["iterations"] == 1 and out["reason"] == "max_iters reached"
    assert torch.equal(out["full"][1:-1, 1:-1], u1)
    assert out["history"][1][2] == math.sqrt(rr1)


def test_cpu_model_surface_and_errors():
    from cuda_mpi_scratch_amd.parallel import DistContext

    m = ConjugateGradient2D(CgConfig(width=24, height=10, dtype="f32", c_center=0.6, c_neighbor=0.1), device="cpu")
    m.set_boundary(top=1.0)
    assert m.graph_status().startswith("off") and "torch references" in m.note()
    assert m.residual()["cells"] == 240
    out = m.solve(1e-5, 200, norm="linf")
    assert out["converged"] and out["norm"] == "linf" and m.iterations_run == out["iterations"]
    assert m.full().shape == (12, 26) and m.field().shape == (10, 24)
    with pytest.raises(ValueError, match="one process"):
        ConjugateGradient2D(CgConfig(width=8, height=8), DistContext(rank=0, world_size=2), device="cpu")
    with pytest.raises(ValueError, match="shape"):
        m.set_source(torch.zeros(24, 10))
    with pytest.raises(ValueError, match="norm"):
        m.solve(1e-8, 5, norm="l1")
