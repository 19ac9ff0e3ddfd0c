"""tests/guided_oracle.py against a per-pair Python loop of the rule in include/gdp.h, one scalar
float32 operation at a time: exact window edges, r = 0, w <= 0, NaN and infinite coordinates, a single
candidate and `unique` ties.  No GPU and no library call."""
import itertools

import numpy as np
import pytest

from guided_oracle import candidates, np_guided, windows
from match_oracle import DESCRIBED_DT, MATCH_DT, NONE

F = np.float32
IDENTITY = np.eye(3, dtype=F)


def records(xy, seed=0, octave=0):
    """One record per (x, y): col = floor(x), dcol = the rest (exact for the values used here)."""
    rng = np.random.default_rng(seed)
    R = np.zeros(len(xy), DESCRIBED_DT)
    for k, (x, y) in enumerate(xy):
        for name, dname, v in (("col", "dcol", x), ("row", "drow", y)):
            if np.isfinite(v) and abs(v) < 2 ** 24:
                R[name][k] = int(np.floor(v))
                R[dname][k] = F(v) - F(np.floor(v))
            else:
                R[dname][k] = F(v)
    R["octave"] = octave
    R["desc"] = rng.integers(0, 256, (len(xy), 128), dtype=np.uint8)
    return R


def loop_guided(Q, T, h, radius, ratio, max_distance, unique):
    """The rule, pair by pair."""
    h = [F(x) for x in np.asarray(h, F).reshape(9)]
    r = F(radius)

    def xy(R, k):
        sc = F(1 << (int(R["octave"][k]) & 31))
        return (F(int(R["col"][k])) + F(R["dcol"][k])) * sc, (F(int(R["row"][k])) + F(R["drow"][k])) * sc

    kept = []
    with np.errstate(all="ignore"):
        for i in range(len(Q)):
            qx, qy = xy(Q, i)
            u = F(F(h[0] * qx) + F(h[1] * qy)) + h[2]
            v = F(F(h[3] * qx) + F(h[4] * qy)) + h[5]
            w = F(F(h[6] * qx) + F(h[7] * qy)) + h[8]
            if not w > 0:
                continue
            sx, sy = F(u / w), F(v / w)
            x0, x1, y0, y1 = F(sx - r), F(sx + r), F(sy - r), F(sy + r)
            best = None
            second = NONE
            for j in range(len(T)):
                tx, ty = xy(T, j)
                if not (x0 <= tx and tx <= x1 and y0 <= ty and ty <= y1):
                    continue
                d = int(((Q["desc"][i].astype(np.int64) - T["desc"][j].astype(np.int64)) ** 2).sum())
                if best is None or d < best[0]:
                    if best is not None:
                        second = min(second, best[0])
                    best = (d, j, tx, ty)
                else:
                    second = min(second, d)
            if best is None:
                continue
            if ratio != 0 and not F(best[0]) < F(F(ratio) * F(ratio)) * F(second):
                continue
            if not best[0] <= max_distance:
                continue
            kept.append((i, best[1], best[0], second, qx, qy, best[2], best[3]))
    if unique:
        kept = [k for k in kept if (k[2], k[0]) == min((o[2], o[0]) for o in kept if o[1] == k[1])]
    out = np.zeros(len(kept), MATCH_DT)
    for n, k in enumerate(kept):
        out[n] = k
    return out


def assert_same(Q, T, h, radius, ratios=(0.0, 0.8), caps=(NONE,)):
    n = 0
    for ratio, cap, unique in itertools.product(ratios, caps, (False, True)):
        got = np_guided(Q, T, h, radius, ratio, cap, unique)
        want = loop_guided(Q, T, h, radius, ratio, cap, unique)
        assert got.tobytes() == want.tobytes(), (radius, ratio, cap, unique, got, want)
        n += len(got)
    return n


def test_window_edges_are_inclusive_and_r_zero_is_an_exact_hit():
    Q = records([(10.0, 20.0)], 1)
    T = records([(7.0, 20.0), (13.0, 20.0), (10.0, 17.0), (10.0, 23.0), (13.0, 23.0), (np.nextafter(F(13), F(14)), 20.0),
                 (np.nextafter(F(7), F(6)), 20.0), (10.0, 20.0)], 2)
    C = candidates(Q, T, IDENTITY, 3.0)
    assert C.tolist() == [[True, True, True, True, True, False, False, True]]
    assert candidates(Q, T, IDENTITY, 0.0).tolist() == [[False] * 7 + [True]]
    assert assert_same(Q, T, IDENTITY, 3.0) > 0 and assert_same(Q, T, IDENTITY, 0.0) > 0
    got = np_guided(Q, T, IDENTITY, 0.0)
    assert len(got) == 1 and int(got["train"][0]) == 7 and int(got["second"][0]) == NONE


def test_w_not_positive_has_no_window():
    Q = records([(5.0, 5.0), (30.0, 5.0), (20.0, 5.0)], 3)
    T = records([(5.0, 5.0), (30.0, 5.0), (20.0, 5.0), (0.0, 0.0)], 4)
    h = np.array([[1, 0, 0], [0, 1, 0], [-1, 0, 20]], F)  # w = 20 - x: positive, negative, zero
    x0, x1, y0, y1, has = windows(Q, h, 100.0)
    assert has.tolist() == [True, False, False]
    assert candidates(Q, T, h, 1e9)[1:].sum() == 0
    assert assert_same(Q, T, h, 1e9) > 0
    assert len(np_guided(Q, T, np.zeros(9, F), 1e9)) == 0  # the fit's "none" record: w = 0 everywhere
    hn = IDENTITY.copy()
    hn[0, 0] = np.nan  # a NaN entry: sx is NaN, every comparison fails
    assert len(np_guided(Q, T, hn, 1e9)) == 0
    assert_same(Q, T, hn, 1e9)


def test_nan_and_infinite_coordinates():
    Q = records([(5.0, 5.0), (np.nan, 5.0), (np.inf, 5.0), (-np.inf, 5.0), (1e30, 5.0)], 5)
    T = records([(5.0, 5.0), (np.nan, 5.0), (5.0, np.nan), (np.inf, 5.0), (-np.inf, 5.0), (1e30, 5.0), (-3.0, 5.0)], 6)
    for radius in (0.0, 1.0, 8.0, 1e9, 3e38):
        C = candidates(Q, T, IDENTITY, radius)
        assert not C[:, 1].any() and not C[:, 2].any() and not C[1].any()  # a NaN is nobody's candidate and has none
        assert_same(Q, T, IDENTITY, radius)
    assert candidates(Q, T, IDENTITY, 8.0)[0].tolist() == [True, False, False, False, False, False, True]
    assert candidates(Q, T, IDENTITY, 0.0)[2].tolist() == [False] * 7  # v = (0 * inf + 5) + 0 is a NaN
    T31 = records([(5.0, 5.0)], 7, octave=31 + 32)  # octave & 31 = 31: the coordinates times 2^31
    assert len(np_guided(Q, T31, IDENTITY, 8.0)) == 0 and len(np_guided(Q, T31, IDENTITY, 3e38)) > 0
    assert_same(Q, T31, IDENTITY, 3e38)


def test_a_single_candidate_passes_the_ratio_test_and_ties_go_to_the_lowest_index():
    Q = records([(5.0, 5.0), (40.0, 40.0)], 8)
    T = records([(5.0, 5.0), (40.0, 40.0), (41.0, 40.0), (40.0, 41.0)], 9)
    T["desc"][2] = T["desc"][1]
    T["desc"][3] = T["desc"][1]
    got = np_guided(Q, T, IDENTITY, 2.0, ratio=0.5, unique=False)
    assert [(int(r["query"]), int(r["train"]), int(r["second"])) for r in got] == [(0, 0, NONE)]  # query 1: second == distance
    got = np_guided(Q, T, IDENTITY, 2.0, unique=False)
    assert int(got["train"][1]) == 1 and int(got["second"][1]) == int(got["distance"][1])
    assert_same(Q, T, IDENTITY, 2.0, ratios=(0.0, 0.5, 1.0), caps=(NONE, 0, int(got["distance"][1]), int(got["distance"][1]) - 1))


def test_unique_keeps_the_nearest_query_and_ties_go_to_the_lowest_query():
    Q = records([(10.0, 10.0), (10.5, 10.0), (10.0, 10.5), (30.0, 30.0)], 10)
    T = records([(10.0, 10.0), (30.0, 30.0), (12.0, 10.0)], 11)
    Q["desc"][0] = T["desc"][0]
    Q["desc"][0, 0] ^= 4  # distance 16
    Q["desc"][1] = Q["desc"][0]  # the same distance: the lowest query wins
    Q["desc"][2] = T["desc"][0]  # distance 0: wins over both
    stats = {}
    both = np_guided(Q, T, IDENTITY, 1.0, unique=False)
    one = np_guided(Q, T, IDENTITY, 1.0, unique=True, stats=stats)
    assert both["train"].tolist() == [0, 0, 0, 1] and one["query"].tolist() == [2, 3] and stats["unique_dropped"] == 2
    tie = np_guided(Q[[0, 1, 3]], T, IDENTITY, 1.0, unique=True)
    assert tie["query"].tolist() == [0, 2]
    # a loser is absent: query 1 also sees train 2 at radius 2, but is not matched to it
    assert np_guided(Q, T, IDENTITY, 2.0, unique=True)["query"].tolist() == [2, 3]
    for radius in (1.0, 2.0):
        assert_same(Q, T, IDENTITY, radius)
        assert_same(Q[[0, 1, 3]], T, IDENTITY, radius)


@pytest.mark.parametrize("seed", range(4))
def test_random_lists_under_a_projective_model(seed):
    rng = np.random.default_rng(seed)
    xy = rng.uniform(-4, 60, (40, 2)).round(2)
    Q = records(xy, seed + 20)
    h = np.array([[0.92, -0.31, 9.5], [0.28, 0.95, -4.25], [1e-3, -2e-3, 1.0]], F)
    with np.errstate(all="ignore"):
        x0, x1, y0, y1, _ = windows(Q, h, 0.0)
    T = records(np.concatenate([np.stack([x0, y0], 1)[:25] + rng.integers(-2, 3, (25, 2)), rng.uniform(0, 60, (30, 2))]), seed + 40)
    T["desc"][:25] = np.clip(Q["desc"][:25].astype(np.int64) + rng.integers(-9, 10, (25, 128)), 0, 255)
    stats = {}
    np_guided(Q, T, h, 6.0, 0.8, stats=stats)
    assert stats["multi"] > 0
    assert assert_same(Q, T, h, 6.0) > 0 and assert_same(Q, T, h, 2.0) > 0
