"""The sum-form reference (the exact association of the GPU sum bodies) agrees
with the per-step Jacobi to rounding: few ulp over a pass, for fp32 and fp64."""
import pytest
import torch

from cuda_mpi_scratch_amd.ops import jacobi_reference_global, jacobi_sum_reference_global


@pytest.mark.parametrize("dtype,steps,tol", [(torch.float64, 16, 1e-14), (torch.float32, 20, 2e-6),
                                             (torch.float32, 32, 2e-6)])
def test_sum_form_reference_close_to_per_step(dtype, steps, tol):
    u = torch.rand(48, 72, generator=torch.Generator().manual_seed(steps), dtype=torch.float64).to(dtype)
    a = jacobi_sum_reference_global(u, steps)
    b = jacobi_reference_global(u, steps)
    assert (a.double() - b.double()).abs().max().item() <= tol


def _bit_view(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


@pytest.mark.parametrize("steps", [4, 3, 5, 16])  # an even ring, odd rings (one column of embedding), a deep one
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_sum_form_block_reference_equals_the_periodic_core(dtype, steps):
    """A ghost-ring array cut from a genuinely periodic field (the ring holds
    the wrapped cells): the block reference's core is the periodic reference,
    bit for bit, whatever the parity of the ring depth."""
    from cuda_mpi_scratch_amd.ops import jacobi_sum_block_reference

    h, w = 9, 14
    u = torch.rand(h, w, generator=torch.Generator().manual_seed(7 + steps), dtype=torch.float64).to(dtype)
    ys = torch.arange(-steps, h + steps) % h
    xs = torch.arange(-steps, w + steps) % w
    full = u[ys][:, xs].contiguous()
    want = jacobi_sum_reference_global(u, steps)
    got = jacobi_sum_block_reference(full, steps)
    assert got.shape == (h, w) and got.dtype == dtype
    assert int((_bit_view(got) != _bit_view(want)).sum()) == 0
    if steps % 2:
        # What the embedding is for: the same array taken as a torus as it
        # stands pairs the odd core columns the other way round.
        naive = jacobi_sum_reference_global(full, steps)[steps:-steps, steps:-steps]
        assert int((_bit_view(naive) != _bit_view(want)).sum()) > 0


def test_sum_form_reference_is_one_scaled_pass():
    """S levels of plain sums then one multiply: with c = 1 it is the raw
    5-point sum recurrence (integers stay exact)."""
    u = torch.randint(0, 4, (8, 12), dtype=torch.int64).double()
    v = jacobi_sum_reference_global(u, 3, c=1.0)
    w = u.clone()
    for _ in range(3):
        w = w + torch.roll(w, 1, 0) + torch.roll(w, -1, 0) + torch.roll(w, 1, 1) + torch.roll(w, -1, 1)
    assert torch.equal(v, w)
