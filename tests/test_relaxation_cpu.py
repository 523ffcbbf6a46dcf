"""Chebyshev relaxation cycles without a GPU: the level table (the C++ function
against its pure-Python twin, the roots, the growth, the errors) and the cycle's
numerics on the torch backend (convergence against plain Jacobi, a 2 x 2 gloo
run, whole-cycle bookkeeping of run() and run_until())."""
import math

import numpy as np
import pytest
import torch

from cuda_mpi_scratch_amd import core, ops
from cuda_mpi_scratch_amd.models.stencil2d import Stencil2D, StencilConfig
from tests.relaxation_worker import BOUNDARY, launch, make

TABLE_CASES = [(96, 64, 0.2, 0.2, 20), (96, 64, 0.2, 0.2, 24), (8192, 8192, 0.2, 0.2, 24), (96, 64, 0.5, 0.125, 12)]


def _rel(a, b):
    return abs(a - b) / max(abs(a), abs(b), 1e-300)


@pytest.mark.parametrize("w,h,c0,c1,M", TABLE_CASES)
def test_table_matches_python_twin(w, h, c0, c1, M):
    t = core().chebyshev_cycle(w, h, c0, c1, M)
    p = ops.chebyshev_cycle(w, h, c0, c1, M)
    assert t["n"] == p["n"] == M and len(t["center"]) == len(t["neighbor"]) == M
    worst = max(max(_rel(a, b) for a, b in zip(t[k], p[k])) for k in ("center", "neighbor"))
    print(f"{w}x{h} {c0}/{c1} M={M}: table rel err {worst:.2e}, growth {t['growth']:.4g} vs {p['growth']:.4g}")
    assert worst <= 1e-12
    assert _rel(t["growth"], p["growth"]) <= 1e-12


@pytest.mark.parametrize("w,h,c0,c1,M", TABLE_CASES)
def test_levels_are_the_chebyshev_roots_in_leja_order(w, h, c0, c1, M):
    t = core().chebyshev_cycle(w, h, c0, c1, M)
    a, b = ops.relaxation_spectrum(w, h, c0, c1)
    roots = (a + b) / 2 + (b - a) / 2 * np.cos(np.pi * (2 * np.arange(M) + 1) / (2 * M))
    omega = np.array(t["neighbor"]) / c1
    got = 1.0 / omega
    assert np.allclose(np.sort(got), np.sort(roots), rtol=1e-12, atol=0), "the levels are not a permutation of the roots"
    # center[l] = 1 - w_l + w_l c0
    assert np.allclose(np.array(t["center"]), 1.0 - omega + omega * c0, rtol=1e-12, atol=1e-12)
    # Leja: the first root has the largest modulus, every next one maximises the
    # product of distances to those taken (ties within rounding allowed).
    assert got[0] == pytest.approx(roots.max(), rel=1e-12)
    for l in range(1, M):
        prod = lambda x: np.prod(np.abs(x - got[:l]))  # noqa: E731
        best = max(prod(x) for x in got[l:])
        assert prod(got[l]) >= best * (1 - 1e-9), f"level {l} is not a Leja point"


@pytest.mark.parametrize("w,h,c0,c1,M", TABLE_CASES)
def test_growth_against_a_denser_sampling(w, h, c0, c1, M):
    t = core().chebyshev_cycle(w, h, c0, c1, M)
    a, b = ops.relaxation_spectrum(w, h, c0, c1)
    omega = np.array(t["neighbor"]) / c1
    # 400 k uniform points plus 400 k Chebyshev-distributed ones, endpoints included.
    k = np.arange(400001) / 400000.0
    x = np.concatenate([a + (b - a) * k, (a + b) / 2 + (b - a) / 2 * np.cos(np.pi * k)])
    dense = np.abs(np.cumprod(1.0 - omega[:, None] * x[None, :], axis=0)).max()
    print(f"{w}x{h} {c0}/{c1} M={M}: growth {t['growth']:.6g}, dense sampling {dense:.6g}")
    assert t["growth"] <= dense * (1 + 1e-12)  # its samples are points of [a, b] too
    assert abs(t["growth"] - dense) <= 0.01 * dense
    # The whole cycle is the scaled Chebyshev polynomial: at most 1 on [a, b].
    assert np.abs(np.prod(1.0 - omega[:, None] * x[None, :], axis=0)).max() <= 1.0 + 1e-9


def test_table_errors():
    C = core()
    for fn in (C.chebyshev_cycle, ops.chebyshev_cycle):
        with pytest.raises(ValueError, match="c_neighbor must not be 0"):
            fn(96, 64, 0.2, 0.0, 20)
        with pytest.raises(ValueError, match="spectrum of I - A must be positive"):
            fn(64, 64, 0.5, 0.25, 20)  # a = 1 - 0.5 - mu < 0 (mu = cos(pi / 65) = 0.9988)
        with pytest.raises(ValueError, match="cycle length"):
            fn(96, 64, 0.2, 0.2, 0)
        with pytest.raises(ValueError, match="cycle length"):
            fn(96, 64, 0.2, 0.2, 33)


def test_config_errors():
    with pytest.raises(ValueError, match="relaxation must be one of"):
        StencilConfig(relaxation="sor")
    with pytest.raises(ValueError, match="needs periodic=False"):
        StencilConfig(relaxation="chebyshev")  # periodic by default
    with pytest.raises(ValueError, match="needs periodic=False"):
        StencilConfig(relaxation="chebyshev", periodic=True, block_fixed_edges=True, time_block=20)
    with pytest.raises(ValueError, match="needs kind='jacobi5'"):
        StencilConfig(relaxation="chebyshev", periodic=False, kind="box")
    StencilConfig(relaxation="none")  # the default, with any other option


# ------------------------------------------------------- the torch backend
ARGS = {"device": "cpu", "w": 96, "h": 64, "dtype": "f64", "time_block": 20, "zero": True}


@pytest.fixture(scope="module")
def converged():
    """run_until(1e-6, 4000) with the cycle on, once for the tests below."""
    st = make(ARGS)
    out = st.run_until(1e-6, 4000)
    return st, out


@pytest.fixture(scope="module")
def plain_reference():
    """Plain Jacobi in float64 from the same start to residual <= 1e-9."""
    w, h = ARGS["w"], ARGS["h"]
    p = torch.zeros(h + 2, w + 2, dtype=torch.float64)
    p[0, 1:-1], p[-1, 1:-1], p[1:-1, 0], p[1:-1, -1] = (BOUNDARY[k] for k in ("top", "bottom", "left", "right"))
    for it in range(200):
        for _ in range(1000):
            p[1:-1, 1:-1] = 0.2 * ((p[:-2, 1:-1] + p[2:, 1:-1]) + (p[1:-1, :-2] + p[1:-1, 2:])) + 0.2 * p[1:-1, 1:-1]
        if ops.residual5_reference(p, 1, 0.2, 0.2)[0] <= 1e-9:
            return p[1:-1, 1:-1].clone(), (it + 1) * 1000
    raise AssertionError("plain Jacobi did not reach 1e-9 in 200 k iterations")


def test_torch_backend_converges_where_plain_jacobi_does_not(converged, plain_reference):
    st, out = converged
    print(f"chebyshev: {out['iterations']} iterations, residual {out['residual']:.3e}; {st.relaxation_note()}")
    assert out["converged"], out["reason"]
    assert out["iterations"] <= 4000 and out["iterations"] % 20 == 0
    assert st.iteration == out["iterations"]
    assert "M = 20" in st.relaxation_note() and "growth" in st.relaxation_note()
    plain = make(dict(ARGS, relaxation="none", time_block=1))
    res = plain.run_until(1e-6, 4000, 400)
    print(f"plain Jacobi: {res['iterations']} iterations, residual {res['residual']:.3e}")
    assert not res["converged"] and res["iterations"] == 4000
    ref, its = plain_reference
    err = (st.core_view().double() - ref).abs().max().item()
    print(f"max |chebyshev - plain Jacobi at 1e-9 ({its} iterations)| = {err:.3e}")
    assert err <= 1e-4


def test_gloo_2x2_equals_one_rank_bitwise(converged):
    st, out = converged
    n = out["iterations"]
    four = launch(4, dict(ARGS, dims="2x2", runs=[n]))
    one = st.core_view().contiguous().numpy().tobytes().hex()
    assert four[0]["grid"] == one
    assert all(r["iteration"] == n and r["cycle"] == 20 for r in four)
    assert all(r["note"] == four[0]["note"] for r in four)


def test_run_needs_whole_cycles_and_run_until_reports_its_rounding():
    st = make(ARGS)
    with pytest.raises(ValueError, match="multiple of the cycle length 20"):
        st.run(30)
    assert st.iteration == 0
    st.run(40)
    assert st.iteration == 40
    out = st.run_until(0.0, 130, 50)  # chunk 50 -> 60 (up), cap 130 -> 120 (down)
    assert out["check_every"] == 60 and out["max_iters"] == 120
    assert out["iterations"] == 120 and not out["converged"]
    assert [h[0] for h in out["history"]] == [0, 60, 120]
    out = st.run_until(0.0, 400)  # default chunk: 16 cycles
    assert out["check_every"] == 16 * 20 and out["max_iters"] == 400 and out["iterations"] == 400
    # Plain Jacobi reports what it was given.
    plain = make(dict(ARGS, relaxation="none", time_block=1))
    out = plain.run_until(0.0, 130, 50)
    assert out["check_every"] == 50 and out["max_iters"] == 130 and out["iterations"] == 130
    assert plain.relaxation_note() == "" and plain.relaxation_info()["cycle"] == 0


def test_automatic_cycle_of_the_torch_backend():
    assert make(dict(ARGS, time_block=0)).cycle == 16                 # fp64
    assert make(dict(ARGS, time_block=0, dtype="f32")).cycle == 24    # fp32
    assert make(dict(ARGS, time_block=12)).cycle == 12
