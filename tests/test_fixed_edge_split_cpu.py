"""kernels::fixed_edge_split (host): the interior / frame split of a tile's core
for time blocking beside fixed edges, exhaustively over small shapes."""
import itertools

import numpy as np
import pytest

from cuda_mpi_scratch_amd import core

SIZES = (1, 7, 24, 40, 41, 100, 264)
DEPTHS = (1, 5, 12, 16, 20, 32)
TOP, BOTTOM, LEFT, RIGHT = 1, 2, 4, 8


def _cases():
    for w, h in itertools.product(SIZES, SIZES):
        for S in DEPTHS:
            if S <= min(w, h):
                yield w, h, S


def test_hold_bits_match_the_kernel_enum():
    C = core()
    assert (C.HOLD_TOP, C.HOLD_BOTTOM, C.HOLD_LEFT, C.HOLD_RIGHT) == (TOP, BOTTOM, LEFT, RIGHT)


@pytest.mark.parametrize("vec", [2, 4])
def test_split_partitions_the_core(vec):
    C = core()
    n = 0
    for w, h, S in _cases():
        for hold in range(16):
            sp = C.fixed_edge_split(w, h, S, vec, hold)
            x0, x1, y0, y1 = sp["interior"]
            frame = sp["frame"]
            assert len(frame) <= 4
            cover = np.zeros((h, w), dtype=np.int32)
            for rx0, rx1, ry0, ry1 in [sp["interior"], *frame]:
                assert 0 <= rx0 <= rx1 <= w and 0 <= ry0 <= ry1 <= h, (w, h, S, vec, hold)
                cover[ry0:ry1, rx0:rx1] += 1
            assert (cover == 1).all(), (w, h, S, vec, hold)
            for rx0, rx1, ry0, ry1 in frame:
                assert rx1 > rx0 and ry1 > ry0, (w, h, S, vec, hold)
            if hold == 0:
                assert (x0, x1, y0, y1) == (0, w, 0, h) and frame == [], (w, h, S, vec)
            if x1 > x0 and y1 > y0:
                # whole vectors (or the core's own right edge on a side that is not held)
                assert x0 % vec == 0, (w, h, S, vec, hold)
                assert x1 % vec == 0 or (x1 == w and not hold & RIGHT), (w, h, S, vec, hold)
                # at least S away from every held side; nothing shrunk on the others
                assert y0 >= S if hold & TOP else y0 == 0
                assert y1 <= h - S if hold & BOTTOM else y1 == h
                assert x0 >= S if hold & LEFT else x0 == 0
                assert x1 <= w - S if hold & RIGHT else x1 == w
                # and no further than the rounding needs
                assert y0 <= S and y1 >= h - S and x0 < S + vec and x1 > w - S - vec
            else:
                # no interior: only a core of at most 2S (+ rounding) cells on a held axis
                assert hold != 0 and frame == [(0, w, 0, h)]
                tight_y = (hold & (TOP | BOTTOM)) and h <= 2 * S
                tight_x = (hold & (LEFT | RIGHT)) and w < 2 * S + 2 * vec
                assert tight_y or tight_x, (w, h, S, vec, hold)
            n += 1
    assert n == 16 * sum(1 for _ in _cases()) and n > 2500


def test_strips_follow_the_documented_layout():
    sp = core().fixed_edge_split(1032, 300, 20, 4, 15)
    assert sp["interior"] == (20, 1012, 20, 280)
    assert sp["frame"] == [(0, 1032, 0, 20), (0, 1032, 280, 300), (0, 20, 20, 280), (1012, 1032, 20, 280)]
    sp = core().fixed_edge_split(262, 200, 5, 4, TOP | LEFT)
    assert sp["interior"] == (8, 262, 5, 200)
    assert sp["frame"] == [(0, 262, 0, 5), (0, 8, 5, 200)]
