"""kernels::balanced_starts (host) with a half-length last group: the shares of a
pipeline pass whose narrow last column group is split into two half-height
sub-groups (the linear space counts ceil(rows / 2) rows for it). The shares
must cover every (group, row) exactly once and keep the modelled cost (rows +
one pipeline fill per chunk) of every workgroup within the function's bounds."""
import numpy as np
import pytest

from cuda_mpi_scratch_amd import core

SHAPES = [  # (groups, rows, blocks, fill): 32768^2, 8192^2 and 16384 x 8192 at S = 24, odd and tiny ones
    (37, 32768, 256, 59), (10, 8192, 256, 59), (19, 8192, 256, 59), (3, 600, 4, 59), (3, 600, 256, 59),
    (2, 97, 256, 59), (2, 7, 256, 59), (1, 1, 256, 59), (1, 2, 8, 59), (1, 193, 3, 59), (5, 1001, 64, 30),
]


def _chunks(starts, groups, rows, last):
    """Per workgroup, the chunks (group, r0, r1) its range of the linear space
    holds, decoded as the kernel decodes it: group = a // rows, and the last
    group ends at `last` rows."""
    out = []
    for a, b in zip(starts, starts[1:]):
        mine = []
        while a < b:
            g = a // rows
            r0 = a - g * rows
            r1 = min(last if g == groups - 1 else rows, r0 + (b - a))
            assert r1 > r0, (g, r0, r1)
            mine.append((g, r0, r1))
            a += r1 - r0
        out.append(mine)
    return out


@pytest.mark.parametrize("groups,rows,blocks,fill", SHAPES)
def test_half_length_last_group_is_covered_once(groups, rows, blocks, fill):
    half = (rows + 1) // 2
    total = (groups - 1) * rows + half
    st = core().balanced_starts(groups, rows, blocks, fill, half)
    assert len(st) == blocks + 1 and st[0] == 0 and st[-1] == total
    assert all(a <= b for a, b in zip(st, st[1:]))
    # Rows of the pass, with the split group's chunk [r0, r1) standing for rows
    # [r0, r1) on sub-group 0 and [r0 + half, min(r1 + half, rows)) on sub-group 1.
    cover = np.zeros((groups, rows), dtype=np.int32)
    for mine in _chunks(st, groups, rows, half):
        for g, r0, r1 in mine:
            if g == groups - 1:
                assert r1 <= half
                cover[g, r0:r1] += 1
                cover[g, min(r0 + half, rows):min(r1 + half, rows)] += 1
            else:
                cover[g, r0:r1] += 1
    assert (cover == 1).all()


@pytest.mark.parametrize("groups,rows,blocks,fill", SHAPES)
def test_half_length_last_group_cost_bounds(groups, rows, blocks, fill):
    """The function's two bounds, in the split space. (1) Never worse than equal
    shares of the same space (the rule it replaced). (2) Its budget T is the
    smallest the greedy walk can meet, and the walk meets any T with
    blocks * (T - 2 fill) >= total + groups * fill: a workgroup leaves at most
    `fill` of its budget unused at its end and pays one fill per chunk, of which
    it has one more per group boundary; so no workgroup costs more than
    ceil((total + groups * fill) / blocks) + 2 fill."""
    half = (rows + 1) // 2
    total = (groups - 1) * rows + half
    cost = lambda st: max(sum(r1 - r0 + fill for _, r0, r1 in mine)  # noqa: E731
                          for mine in _chunks(st, groups, rows, half))
    new = cost(core().balanced_starts(groups, rows, blocks, fill, half))
    share = -(-total // blocks)
    assert new <= cost([min(w * share, total) for w in range(blocks + 1)])
    assert new <= -(-(total + groups * fill) // blocks) + 2 * fill


def test_last_rows_default_is_the_whole_group():
    C = core()
    assert C.balanced_starts(9, 8192, 256, 47, 0) == C.balanced_starts(9, 8192, 256, 47)
    assert C.balanced_starts(9, 8192, 256, 47, 8192) == C.balanced_starts(9, 8192, 256, 47)
    # 32768^2 at S = 24: 36.5 groups of rows instead of 37 over 256 workgroups.
    st = C.balanced_starts(37, 32768, 256, 59, 16384)
    assert st[-1] == 36 * 32768 + 16384
