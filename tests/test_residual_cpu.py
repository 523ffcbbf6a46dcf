"""Residual norms and run_until without a GPU: the float64 CPU reference
(ops.residual5_reference) on cases computed by hand, and Stencil2D.residual() /
run_until() on the torch backend, on one rank and on a 2 x 2 gloo grid."""
import math

import pytest
import torch

from cuda_mpi_scratch_amd import ops
from cuda_mpi_scratch_amd.models.stencil2d import Stencil2D, StencilConfig
from tests.residual_worker import boundary, launch, padded, reference_history

TOL64 = 1e-14  # the project's fp64 tolerance for fields in [0, 1)


def test_reference_hand_computed_3x3():
    # Core 1 x 1 (value 2) inside a 3 x 3 view: n = 1, s = 3, w = 5, e = 7,
    # corners 100 (never read). A u = 0.5 * 2 + 0.125 * 16 = 3: r = 1.
    full = torch.tensor([[100.0, 1.0, 100.0], [5.0, 2.0, 7.0], [100.0, 3.0, 100.0]], dtype=torch.float64)
    linf, l2 = ops.residual5_reference(full, 1, 0.5, 0.125)
    assert linf == 1.0 and l2 == 1.0
    # 3 x 3 core of ones inside a ring of zeros, 0.2 / 0.2: the centre keeps its
    # value (5 * 0.2 = 1), an edge cell loses one neighbour (-0.2), a corner two (-0.4).
    full = torch.zeros(5, 5, dtype=torch.float64)
    full[1:4, 1:4] = 1.0
    linf, l2 = ops.residual5_reference(full, 1, 0.2, 0.2)
    assert abs(linf - 0.4) <= 1e-15
    assert abs(l2 - math.sqrt(4 * 0.16 + 4 * 0.04)) <= 1e-15
    # A deeper ring: only the layer beside the core enters.
    deep = torch.full((9, 9), float("nan"), dtype=torch.float64)
    deep[2:7, 2:7] = full
    deep[2, 2] = deep[2, 6] = deep[6, 2] = deep[6, 6] = float("nan")  # the corners of the 1-deep ring
    assert ops.residual5_reference(deep, 3, 0.2, 0.2) == (linf, l2)
    with pytest.raises(ValueError, match="no ghost ring"):
        ops.residual5_reference(full, 0)


def test_reference_linear_field_is_harmonic():
    h, w = 12, 9
    y = torch.arange(-1, h + 1, dtype=torch.float64)
    full = (3.0 + 0.25 * y)[:, None].expand(h + 2, w + 2).contiguous()  # linear in y, boundary values matching
    linf, l2 = ops.residual5_reference(full, 1, 0.2, 0.2)
    assert linf <= 4 * TOL64 * full.abs().max().item() and l2 <= 4 * TOL64 * full.abs().max().item() * math.sqrt(w * h)


def _cpu_solver(w, h, dtype="f64", periodic=False, seed=3):
    st = Stencil2D(StencilConfig(global_width=w, global_height=h, dims="1x1", dtype=dtype, periodic=periodic,
                                 seed=seed), device="cpu")
    if not periodic:
        st.set_boundary(**boundary(w, h))
    return st


def test_cpu_residual_equals_reference():
    w, h = 48, 32
    st = _cpu_solver(w, h)
    bnd = boundary(w, h)
    want = ops.residual5_reference(padded(st.gather_global(), bnd), 1)
    before = st.core_view().clone()
    got = st.residual()
    assert (got["linf"], got["l2"], got["cells"]) == (want[0], want[1], w * h)
    assert torch.equal(st.core_view(), before)
    st.run(7)
    want = ops.residual5_reference(padded(st.gather_global(), bnd), 1)
    got = st.residual()
    assert (got["linf"], got["l2"]) == want
    per = _cpu_solver(w, h, periodic=True)
    per.run(3)
    assert (per.residual()["linf"], per.residual()["l2"]) == ops.residual5_reference(padded(per.gather_global()), 1)


_HIST = {}


def _history(w, h, every, checks, periodic):
    key = (w, h, every, checks, periodic)
    if key not in _HIST:
        st = _cpu_solver(w, h, periodic=periodic)
        _HIST[key] = reference_history(st.gather_global(), every, checks, None if periodic else boundary(w, h))
    return _HIST[key]


def test_cpu_run_until_stopping_rule_fixed_edges():
    w, h, every = 48, 32, 60
    hist = [x[0] for x in _history(w, h, every, 18, False)]
    tol = math.sqrt(hist[16] * hist[17])
    print(f"reference linf at 960 / 1020: {hist[16]:.6g} / {hist[17]:.6g}, tol {tol:.6g}")
    assert hist[16] / tol >= 1.05 and tol / hist[17] >= 1.05  # the reference's own margin
    st = _cpu_solver(w, h)
    out = st.run_until(tol, 5000, every)
    assert out["converged"] and out["iterations"] == 1020 and out["checks"] == 18, out
    assert st.iteration == 1020
    assert abs(out["residual"] - hist[17]) <= 2 * TOL64 * 100
    assert [it for it, _, _ in out["history"]] == list(range(0, 1021, every))
    assert "converged" in out["reason"] and out["norm"] == "linf"


def test_cpu_run_until_l2_cap_and_non_finite():
    w, h, every = 48, 32, 60
    l2 = [x[1] for x in _history(w, h, every, 18, False)]
    tol = math.sqrt(l2[16] * l2[17])
    assert l2[16] / tol >= 1.05 and tol / l2[17] >= 1.05
    st = _cpu_solver(w, h)
    out = st.run_until(tol, 5000, every, norm="l2")
    assert out["converged"] and out["iterations"] == 1020 and out["checks"] == 18, out
    assert abs(out["residual"] - l2[17]) <= 2 * TOL64 * 100 * math.sqrt(w * h)
    st = _cpu_solver(w, h)
    out = st.run_until(0.0, 120, every)
    assert not out["converged"] and out["iterations"] == 120 and out["checks"] == 3 and "max_iters" in out["reason"]
    st = _cpu_solver(w, h)
    st.core_view()[5, 7] = float("nan")
    out = st.run_until(1e-3, 600, every)
    assert not out["converged"] and out["iterations"] == 0 and "non-finite" in out["reason"], out


def test_cpu_run_until_already_converged_and_default_chunk():
    w, h = 24, 16
    st = Stencil2D(StencilConfig(global_width=w, global_height=h, dims="1x1", dtype="f64", periodic=False), device="cpu")
    st.core_view().fill_(1.0)
    st.set_boundary(top=1.0, bottom=1.0, left=1.0, right=1.0)
    out = st.run_until(1e-12, 100)
    assert out["converged"] and out["iterations"] == 0 and out["checks"] == 1 and out["residual"] == 0.0
    st = _cpu_solver(w, h)
    out = st.run_until(0.0, 40)  # check_every = 0: 16 x the time block (1 on the torch backend)
    assert [it for it, _, _ in out["history"]] == [0, 16, 32, 40]


def test_cpu_bad_arguments_raise():
    st = _cpu_solver(24, 16)
    with pytest.raises(ValueError, match="tol"):
        st.run_until(-1.0, 10)
    with pytest.raises(ValueError, match="max_iters"):
        st.run_until(1.0, -1)
    with pytest.raises(ValueError, match="norm"):
        st.run_until(1.0, 10, norm="l1")
    box = Stencil2D(StencilConfig(global_width=24, global_height=16, dims="1x1", kind="box", box_weights=[1 / 9] * 9),
                    device="cpu")
    with pytest.raises(ValueError, match="box"):
        box.residual()
    with pytest.raises(ValueError, match="box"):
        box.run_until(1.0, 10)


def test_cpu_2x2_gloo_agrees_with_one_rank():
    w, h, every = 48, 32, 60
    hist = [x[0] for x in _history(w, h, every, 18, False)]
    tol = math.sqrt(hist[16] * hist[17])
    args = {"device": "cpu", "w": w, "h": h, "dtype": "f64", "seed": 3, "tol": tol, "max_iters": 5000,
            "check_every": every}
    one = launch(1, dict(args, dims="1x1"))[0]
    four = launch(4, dict(args, dims="2x2"))
    assert one["until"]["converged"] and one["until"]["iterations"] == 1020
    for r in four:
        assert r["until"] == four[0]["until"] and r["first"] == four[0]["first"], r
        assert r["iteration"] == 1020
    assert four[0]["until"]["iterations"] == one["until"]["iterations"]
    assert four[0]["until"]["checks"] == one["until"]["checks"] == 18
    assert four[0]["until"]["residual"] == one["until"]["residual"]  # a max: order-free, the fields are bitwise equal
    assert four[0]["first"]["cells"] == w * h
    assert abs(four[0]["first"]["l2"] - one["first"]["l2"]) <= 1e-12 * one["first"]["l2"]
    assert four[0]["grid"] == one["grid"]
