"""The descriptor oracle (tests/describe_oracle.py) checked on the CPU: against a float64 SIFT
descriptor with real cos, sin, atan2 and exp, the polynomial A against atan, the rotation table, the
bins of constant gradients in closed form, and every drop and reject path.  No GPU, no library: the
tables are the formulas'."""
import functools

import numpy as np
import pytest

from describe_oracle import (A_COEF, ANGLES, F, float64_descriptor, formula_rotation, formula_tables, formula_weights,
                             np_describe, np_octant, np_orientation, oriented_records, radius, tree_sum_squares)
from extrema_oracle import packed_size

S3, N = 3, 64


@functools.lru_cache(maxsize=None)
def blurred_level():
    """A random 64 x 64 level box-blurred 5 x 5 (edges repeated), as one octave of S = 3 whose DoG
    levels are zero: L = level S+2 exactly, for every s."""
    x = np.random.default_rng(11).standard_normal((N, N)).astype(F) * F(40.0)
    for axis in (0, 1):
        pad = np.pad(x, [(2, 2) if a == axis else (0, 0) for a in (0, 1)], mode="edge")
        x = sum(np.take(pad, range(k, k + N), axis=axis) for k in range(5)) * F(0.2)
    D = np.zeros((S3 + 3, N, N), F)
    D[S3 + 2] = x
    D.setflags(write=False)
    return D


def describe_one_octave(D, recs):
    S = D.shape[0] - 3
    rows, cols = D.shape[1:]
    return np_describe(np.ascontiguousarray(D).ravel(), rows, cols, S, 1, recs, *formula_tables(S))


def test_rule_against_the_float64_descriptor():
    """36 + 12 in-image points of s = 1..3 (window never clipped), random angles plus 0, 90, 180,
    270: no byte differs by more than 1 from the float64 descriptor, and at most 10 % differ at all
    (a wrong bin layout cannot pass that)."""
    D = blurred_level()
    rng = np.random.default_rng(5)
    points = [(1 + k % 3, int(rng.integers(14, N - 14)), int(rng.integers(14, N - 14)), float(F(rng.uniform(0, 360))))
              for k in range(36)]
    points += [(s, 20 + 7 * s, 40 - 5 * s, a) for s in (1, 2, 3) for a in (0.0, 90.0, 180.0, 270.0)]
    recs = oriented_records(points)
    out, why = describe_one_octave(D, recs)
    assert why == ["ok"] * len(points) and len(points) >= 36
    got = {(t[1], t[3], t[4], t[10]): np.array(t[14], np.int64) for t in out}
    assert len(got) == len(points)
    differ = total = worst = 0
    for s, r, c, a in points:
        want = float64_descriptor(D[S3 + 2], s, r, c, a).astype(np.int64)
        mine = got[(s, r, c, int(F(a).view(np.uint32)))]
        assert want.max() > 40 and (want > 0).sum() > 40  # a real descriptor, not a degenerate one
        worst = max(worst, int(np.abs(want - mine).max()))
        differ += int((want != mine).sum())
        total += want.size
    print(f"{differ} of {total} bytes differ from float64 ({100.0 * differ / total:.2f} %), largest difference {worst}")
    assert worst <= 1
    assert differ <= 0.10 * total


def test_polynomial_against_atan():
    t = np.linspace(0.0, 1.0, 2_000_001).astype(F)
    a = np_octant(t)
    assert a.dtype == np.float32
    err = np.abs(a.astype(np.float64) - np.arctan(t.astype(np.float64)) * 4.0 / np.pi).max()
    print(f"A(t): largest error {err:.3e} bins over {t.size} t; A(1) = {a[-1]!r}")
    assert err <= 2.0 ** -16
    assert np.all(np.diff(a) >= 0) and a[0] == 0 and a.max() <= 1.0
    assert A_COEF.view(np.uint32).tolist() == [0x3fa2f890, 0xbed8d61d, 0x3e7c5661, 0xbe17cbe9, 0x3d89486e, 0xbc74784e]


def test_orientation_of_the_axes_and_diagonals():
    gu = np.array([1, 1, 0, -1, -1, -1, 0, 1, 0], F)
    gv = np.array([0, 1, 1, 1, 0, -1, -1, -1, 0], F)
    ob = np_orientation(gu, gv)
    assert ob[[0, 2, 4, 6]].tolist() == [0.0, 2.0, 4.0, 6.0] and ob[8] == 6.0  # (0, 0): q = 3, w8 = 0
    assert np.abs(ob[[1, 3, 5, 7]] - np.array([1, 3, 5, 7])).max() < 3e-6
    assert np_orientation(np.array([1], F), np.array([-1e-30], F))[0] < 8.0  # just under a full turn: never 8


def test_rotation_table():
    C, S = formula_rotation()
    assert C.dtype == np.float32 and C.size == S.size == ANGLES
    assert [float(C[a]) for a in (0, 360, 720, 1080)] == [1.0, 0.0, -1.0, 0.0]
    assert [float(S[a]) for a in (0, 360, 720, 1080)] == [0.0, 1.0, 0.0, -1.0]
    a = np.arange(ANGLES)
    assert np.array_equal(C, S[(a + 360) % ANGLES])  # cos(x) = sin(x + 90 degrees), bit for bit
    assert np.array_equal(C[(a + 720) % ANGLES], -C) and np.array_equal(S[(a + 720) % ANGLES], -S)
    exact = np.cos(a * np.pi / 720.0)
    assert np.abs(C.astype(np.float64) - exact).max() < 6e-8 and np.abs(C * C + S * S - 1).max() < 2e-7


def test_tables_follow_the_formulas():
    assert [radius(s) for s in range(1, 10)] == [11, 7, 5, 4, 4, 3, 3, 2, 2]
    for s in range(1, 10):
        w = formula_weights(s)
        assert w.size == 2 * radius(s) ** 2 + 1 <= 243 and w[0] == 1.0 and np.all(np.diff(w) < 0)
    v = np.arange(128, dtype=F).reshape(1, 128)
    assert tree_sum_squares(v)[0] == F((np.arange(128.0) ** 2).sum())  # small integers: every partial sum exact


def gradient_octave(S, rows, cols, s, a, b):
    """Level S+2 = a * col, level S+1 = b * row, levels s..S zero, the levels below s NaN: L = a col +
    b row exactly, (gx, gy) = (2a, 2b) at every sample, and a read below s rejects everything."""
    D = np.zeros((S + 3, rows, cols), F)
    D[:s] = np.nan
    D[S + 2] = F(a) * np.arange(cols, dtype=F)[None, :]
    D[S + 1] = F(b) * np.arange(rows, dtype=F)[:, None]
    return D


@pytest.mark.parametrize("s", [1, 2, 3])
def test_constant_gradient_fills_one_orientation_bin(s):
    rows = cols = 40
    recs = oriented_records([(s, 20, 20, 0.0)])
    out, why = describe_one_octave(gradient_octave(3, rows, cols, s, 1, 0), recs)  # (gx, gy) = (2, 0)
    assert why == ["ok"]
    d = np.array(out[0][14]).reshape(4, 4, 8)
    assert (d[:, :, 0] > 0).all() and not d[:, :, 1:].any()
    assert np.array_equal(d[:, :, 0], d[::-1, :, 0]) and np.array_equal(d[:, :, 0], d[:, ::-1, 0])  # the window is symmetric
    out, why = describe_one_octave(gradient_octave(3, rows, cols, s, 0, 1), recs)  # (0, 2): 90 degrees on
    d2 = np.array(out[0][14]).reshape(4, 4, 8)
    assert np.array_equal(d2[:, :, 2], d[:, :, 0]) and not d2[:, :, [0, 1, 3, 4, 5, 6, 7]].any()
    # the keypoint turned with the gradient: the gradient is back in bin 0
    out, why = describe_one_octave(gradient_octave(3, rows, cols, s, 0, 1), oriented_records([(s, 20, 20, 90.0)]))
    d3 = np.array(out[0][14]).reshape(4, 4, 8)
    assert np.array_equal(d3, d)
    assert out[0][5:10] == tuple(int(F(x).view(np.uint32)) for x in (1.5, 0.25, -0.125, 0.5, 2.5))  # copied through


def test_every_reject_and_drop_path_returns_none():
    rows = cols = 40
    D = gradient_octave(3, rows, cols, 1, 1, 1)
    ok = oriented_records([(1, 20, 20, 45.0)])
    assert describe_one_octave(D, ok)[1] == ["ok"]
    nan = D.copy()
    nan[3 + 2, 22, 25] = np.nan  # inside the rotated window of (20, 20)
    assert describe_one_octave(nan, ok) == ([], ["nonfinite"])
    inf = D.copy()
    inf[3 + 1, 18, 17] = np.inf
    assert describe_one_octave(inf, ok) == ([], ["nonfinite"])
    assert describe_one_octave(np.zeros_like(D), ok) == ([], ["flat"])
    tiny = gradient_octave(3, rows, cols, 1, 1, 0) * F(2.0 ** -149)  # gx*gx underflows: every m is +0
    assert describe_one_octave(tiny, ok) == ([], ["flat"])
    for point in [(1, 0, 20, 0.0), (1, rows - 1, 20, 0.0), (1, 20, 0, 0.0), (1, 20, cols - 1, 0.0), (0, 20, 20, 0.0),
                  (4, 20, 20, 0.0), (1, 20, 20, 360.0), (1, 20, 20, -0.25), (1, 20, 20, float("nan")),
                  (1, 20, 20, float("inf"))]:
        assert describe_one_octave(D, oriented_records([point])) == ([], ["dropped"]), point
    assert describe_one_octave(D, oriented_records([(1, 20, 20, 0.0)], octave=1)) == ([], ["dropped"])
    # the same NaN is outside the window of (5, 5) at s = 2 (R = 7 reads rows and columns up to 13)
    assert describe_one_octave(nan, oriented_records([(2, 5, 5, 0.0)]))[1] == ["ok"]
    # angle 359.9: a = 1440 wraps to 0
    a, b = describe_one_octave(D, oriented_records([(1, 20, 20, 359.9)])), describe_one_octave(D, oriented_records([(1, 20, 20, 0.0)]))
    assert a[0][0][14] == b[0][0][14]


def test_border_clipped_window():
    rows, cols = 24, 40
    D = gradient_octave(3, rows, cols, 1, 1, 0)
    clipped = []
    recs = oriented_records([(1, 1, cols - 2, 0.0), (1, 12, 20, 0.0)])
    out, why = np_describe(D.ravel(), rows, cols, 3, 1, recs, *formula_tables(3), clipped_out=clipped)
    assert why == ["ok", "ok"] and clipped == [True, True]  # R = 11 also clips the 24-row level's centre
    corner = np.array([t for t in out if t[3] == 1][0][14]).reshape(4, 4, 8)
    # rows above r = 1 and columns right of c = cols - 2 hold no samples: those spatial bins stay empty
    assert not corner[0].any() and not corner[:, 3].any() and corner[2:, :2, 0].all() and not corner[:, :, 1:].any()
