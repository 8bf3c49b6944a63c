"""The facts of the path-flattening rule (include/skf.h, Path flattening) asserted on its host restatement,
tests/flatten_reference.py, without a GPU: the error bound, the degenerate cubics, monotonicity, the saturation and the joins.
tests/test_gpu_flatten.py holds the device to the restatement bit for bit."""
import numpy as np
import pytest

import flatten_reference as fr

TOLS = (0.05, 0.25, 1.0)


@pytest.fixture(scope="module")
def cubics():
    return fr.random_cubics(300)


@pytest.mark.parametrize("tol", TOLS)
def test_polyline_stays_within_tol_of_the_curve(cubics, tol):
    """tol bounds the chord error of the exact pieces; 2^-23 * max|coord| is the rounding of a row to float32 (half an ulp a
    coordinate, at most 2^-24 * |coord| each, taken generously)."""
    n = fr.pieces(cubics, np.ones(len(cubics), np.int32), tol)
    worst = 0.0
    for p, k in zip(cubics, n):
        dev = fr.deviation(p, int(k))
        bound = tol + 2.0 ** -23 * np.abs(p).max()
        worst = max(worst, dev / bound)
        assert dev <= bound, (p.tolist(), int(k), dev, bound)
    print("tol %g: n from %d to %d, worst deviation %.3f of the bound" % (tol, n.min(), n.max(), worst))
    assert n.min() >= 2 and n.max() < 400


def test_a_line_a_straight_cubic_and_a_point_cubic_have_one_piece():
    line = fr.line_segment((3, 4), (500, -200))
    wild = np.array([(0, 0), (900, -900), (-900, 900), (10, 10)], np.float64)               # kind 0: p1 and p2 do not count
    straight = np.array([(0, 0), (10, 20), (20, 40), (30, 60)], np.float64)               # evenly spaced: both second differences 0
    point = np.repeat(np.array([(7.5, -2.25)]), 4, axis=0)
    ctrl = np.stack([line, wild, straight, point])
    assert fr.pieces(ctrl, [0, 0, 1, 1], 1e-6).tolist() == [1, 1, 1, 1]
    assert fr.pieces(ctrl, [0, 2, 1, 1], 1e-6).tolist() == [1, 1, 1, 1]                   # a kind other than 0 or 1 is a line
    rows = fr.flatten_subpath(ctrl[1:2], [0], 0.5)
    assert rows.tolist() == [[0.0, 0.0], [10.0, 10.0]]
    assert fr.pieces(wild[None], [1], 0.5)[0] > 10


def test_pieces_grow_with_the_precision_asked_for(cubics):
    kind = np.ones(len(cubics), np.int32)
    before = fr.pieces(cubics, kind, 4.0)
    for tol in (2.0, 1.0, 0.5, 0.1, 0.01, 1e-4):
        n = fr.pieces(cubics, kind, tol)
        assert (n >= before).all()
        before = n
    assert (before > fr.pieces(cubics, kind, 4.0)).all()
    # a quarter of the tolerance doubles n, up to the ceiling of the smallest integer
    n1, n4 = fr.pieces(cubics, kind, 1.0), fr.pieces(cubics, kind, 0.25)
    assert ((n4 >= 2 * n1 - 1) & (n4 <= 2 * n1)).all()


def test_piece_count_is_the_smallest_that_passes_and_saturates():
    for n in (2, 3, 63, 64, 65, 1000, 4095, 4096):
        assert fr.pieces(fr.bump(n, 0.25)[None], [1], 0.25)[0] == n, n
    huge = np.array([(0, 0), (1e9, 1e9), (-1e9, 1e9), (0, 0)], np.float64)
    nan = np.array([(0, 0), (np.nan, 1), (2, 1), (3, 0)], np.float64)
    half = np.array([(0, 0), (1, 1), (2, np.nan), (3, 0)], np.float64)                      # a NaN in one second difference only
    inf = np.array([(0, 0), (1e200, 0), (2, 1), (3, 0)], np.float64)                      # ax * ax overflows
    assert fr.pieces(np.stack([huge, nan, half, inf]), [1, 1, 1, 1], 0.25).tolist() == [fr.MAX_N] * 4
    rows = fr.flatten_subpath(huge[None], [1], 0.25)
    assert len(rows) == fr.MAX_N + 1 and rows[0].tolist() == [0, 0] and rows[-1].tolist() == [0, 0]
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="tol"):
            fr.c_of(bad)


def test_joins_repeat_no_row_and_skip_none():
    ctrl, kind, offsets = fr.random_subpaths([5, 0, 1, 9], line_every=3)
    assert offsets.tolist() == [0, 5, 5, 6, 15] and set(kind.tolist()) == {0, 1}
    parts = fr.flatten(ctrl, kind, offsets, 0.25)
    n = fr.pieces(ctrl, kind, 0.25)
    assert [len(p) for p in parts] == [1 + n[:5].sum(), 0, 1 + n[5], 1 + n[6:].sum()]
    first = parts[0]
    ends = np.cumsum(n[:5])
    assert fr.same_bits(first[0], ctrl[0, 0].astype(np.float32))
    assert fr.same_bits(first[ends], ctrl[:5, 3].astype(np.float32))            # every segment's end, copied
    assert (np.abs(np.diff(first, axis=0)).sum(axis=1) > 0).all()              # no row twice in a row
    # a subpath's rows do not depend on its neighbours, and the clamp of the ranges defines what garbage offsets mean
    assert fr.same_bits(parts[3], fr.flatten_subpath(ctrl[6:], kind[6:], 0.25))
    clamped = fr.flatten(ctrl, kind, np.array([-4, 5, 99, 7]), 0.25)
    assert fr.same_bits(clamped[0], parts[0]) and len(clamped[1]) == 1 + n[5:].sum() and len(clamped[2]) == 0


def test_rows_are_de_casteljau_in_the_stated_order():
    p = np.array([(0.1, 0.2), (10.3, 40.7), (55.5, -3.3), (70.9, 20.1)], np.float64)
    n = int(fr.pieces(p[None], [1], 0.25)[0])
    rows = fr.segment_rows(p, n)
    j = n // 3
    t = np.float64(j) / np.float64(n)
    for axis in (0, 1):
        a, b, c, d = p[:, axis]
        q0, q1, q2 = a + t * (b - a), b + t * (c - b), c + t * (d - c)
        r0, r1 = q0 + t * (q1 - q0), q1 + t * (q2 - q1)
        assert rows[j - 1, axis] == np.float32(r0 + t * (r1 - r0))
    assert np.abs(rows - fr.bernstein(p, np.arange(1, n + 1) / n)).max() < 1e-4
