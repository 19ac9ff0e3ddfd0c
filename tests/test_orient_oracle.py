"""The orientation oracle (tests/orient_oracle.py) checked on the CPU, without the library: the
boundary table, the bins of the axes and diagonals, agreement with atan2 away from the boundaries,
the closed form of the gradient pyramids, rejection on NaN and inf, and border clipping."""
import math

import numpy as np
import pytest

from extrema_oracle import ODD, F, smooth_pyramid, tie_pyramid, want
from orient_oracle import (BINS, DIRECTIONS, T, T_BITS, as_multiset, formula_tables, formula_weights, gaussian_level,
                           gradient_pyramid, np_bin, np_orient, radius, refined_from, refined_records)
from refine_oracle import records_from_set

GS, GROWS, GCOLS = 3, 24, 40


def bits(x):
    return int(F(x).view(np.uint32))


def test_boundary_table_is_the_nearest_float32_to_the_tangents():
    assert T_BITS == (0x3e348f0f, 0x3eba5a4e, 0x3f13cd3a, 0x3f56cf3c, 0x3f988b62, 0x3fddb3d7, 0x402fd6ac, 0x40b57b24)
    for k in range(1, 9):
        exact = math.tan(math.radians(10 * k))
        t = T[k - 1]
        assert bits(t) == bits(np.float32(exact))
        lo, hi = np.nextafter(t, F(-np.inf)), np.nextafter(t, F(np.inf))
        assert abs(float(t) - exact) <= min(abs(float(lo) - exact), abs(float(hi) - exact))


def test_bins_of_the_axes_and_diagonals():
    for (gx, gy), want_bin in DIRECTIONS:
        assert int(np_bin(F(gx), F(gy))) == want_bin, (gx, gy)
    assert [b for _, b in DIRECTIONS] == [0, 9, 18, 27, 4, 13, 22, 31]
    # the quadrants are half open: every axis belongs to the quadrant it starts, whatever the zero's sign
    assert int(np_bin(F(1), F(-0.0))) == 0 and int(np_bin(F(-0.0), F(1))) == 9
    assert int(np_bin(F(-1), F(0.0))) == 18 and int(np_bin(F(0.0), F(-1))) == 27


def test_bins_agree_with_atan2_away_from_the_boundaries():
    rng = np.random.default_rng(11)
    g = rng.standard_normal((20000, 2)).astype(np.float32) * F(100)
    deg = np.degrees(np.arctan2(g[:, 1].astype(np.float64), g[:, 0].astype(np.float64))) % 360.0
    away = np.abs(deg / 10.0 - np.round(deg / 10.0)) * 10.0 > 1e-4
    assert away.sum() > 19900
    got = np_bin(g[:, 0], g[:, 1])
    assert np.array_equal(got[away], np.floor(deg[away] / 10.0).astype(np.int64))
    assert got.min() == 0 and got.max() == BINS - 1


def test_radius_and_weights():
    assert [radius(s) for s in range(1, 10)] == [5, 3, 3, 2, 2, 2, 2, 1, 1]
    assert all(radius(s) >= 1 and radius(s) == -(-9 // (s + 1)) for s in range(1, 61))  # ceil(3 * 1.5 * 2 / (s + 1))
    for s in (1, 2, 3, 5):
        w = formula_weights(s)
        assert w.dtype == np.float32 and w.size == 2 * radius(s) ** 2 + 1 and w[0] == 1.0
        assert np.all(np.diff(w) < 0) and w[-1] > 1e-8  # far from the denormals


def test_gaussian_level_is_the_suffix_sum_in_the_rules_order():
    D = np.random.default_rng(3).standard_normal((GS + 3, 5, 7)).astype(np.float32)
    for s in range(1, GS + 1):
        L = D[GS + 2]
        for t in range(GS + 1, s - 1, -1):
            L = L + D[t]
        assert np.array_equal(gaussian_level(D, GS, s), L)
    poisoned = D.copy()
    poisoned[:2] = np.nan  # levels below s = 2 are never read
    assert np.array_equal(gaussian_level(poisoned, GS, 2), gaussian_level(D, GS, 2))


@pytest.mark.parametrize("s", [1, 2, 3])
def test_closed_form_of_the_gradient_pyramids(s):
    points = [(s, 12, 20), (s, 1, 1), (s, GROWS - 2, GCOLS - 2), (s, 8, 30)]
    recs = refined_records(points)
    for (a, b), want_bin in DIRECTIONS:
        D = gradient_pyramid(GS, GROWS, GCOLS, s, a, b)
        got, why = np_orient(D.ravel(), GROWS, GCOLS, GS, 1, recs, formula_tables(GS))
        assert why == ["ok"] * 4 and len(got) == 4
        for t in got:
            assert t[12] == want_bin and t[13] == 1 and t[10] == bits(10.0 * want_bin)
            assert t[5:10] == (bits(1.5), bits(0.25), bits(-0.125), bits(0.5), bits(2.5))  # copied through
        # the peak is 0.375 of the one bin's sum; the corner keypoints see a quarter of the window
        peaks = {t[3:5]: np.array([t[11]], np.uint32).view(np.float32)[0] for t in got}
        assert peaks[(12, 20)] == peaks[(8, 30)] > peaks[(1, 1)] > 0
        R, w = radius(s), formula_weights(s)
        mag = np.sqrt(F(2 * a) * F(2 * a) + F(2 * b) * F(2 * b))
        hist = F(0)
        for dr in range(-R, R + 1):
            part = F(0)
            for dc in range(-R, R + 1):
                part = part + mag * w[dr * dr + dc * dc]
            hist = hist + part
        assert bits(peaks[(12, 20)]) == bits(((F(0) + F(0)) * F(0.0625) + (F(0) + F(0)) * F(0.25)) + hist * F(0.375))


def test_a_level_below_s_is_what_rejects():
    D = gradient_pyramid(GS, GROWS, GCOLS, 2, 1, 0)
    recs = refined_records([(1, 12, 20), (2, 12, 20)])  # scale 1 reads level 1, which is NaN here
    got, why = np_orient(D.ravel(), GROWS, GCOLS, GS, 1, recs, formula_tables(GS))
    assert why == ["nonfinite", "ok"] and len(got) == 1 and got[0][1] == 2


@pytest.mark.parametrize("poison", [np.nan, np.inf, -np.inf])
def test_rejection_on_nan_and_inf(poison):
    D = gradient_pyramid(GS, GROWS, GCOLS, 1, 1, 1)
    D[GS, 12, 20] = poison  # enters L of every scale <= S
    near = refined_records([(3, 12, 20), (3, 12, 24), (3, 12, 25), (1, 6, 20), (1, 5, 20)])
    got, why = np_orient(D.ravel(), GROWS, GCOLS, GS, 1, near, formula_tables(GS))
    # R_3 = 3: a window reaches 4 samples (3 + the gradient's 1); R_1 = 5 reaches 6
    assert why == ["nonfinite", "nonfinite", "ok", "nonfinite", "ok"]
    assert [t[3:5] for t in got] == [(5, 20), (12, 25)]
    flat = np.zeros((GS + 3, GROWS, GCOLS), F)
    got, why = np_orient(flat.ravel(), GROWS, GCOLS, GS, 1, near, formula_tables(GS))
    assert got == [] and why == ["flat"] * 5


def test_border_clipping_and_the_shared_pyramids():
    H, W, S, O = ODD
    rec = refined_from(records_from_set(want("smooth", ODD)[0]))
    clipped = []
    got, why = np_orient(smooth_pyramid(ODD), H, W, S, O, rec, formula_tables(S), clipped_out=clipped)
    assert len(rec) > 500 and why.count("ok") == len(rec) and sum(clipped) > 100 and not all(clipped)
    per_input = {}
    for t in got:
        per_input.setdefault(t[:5], []).append(t)
    assert len(per_input) == len(rec)
    for group in per_input.values():
        assert all(t[13] == len(group) for t in group) and 1 <= len(group) <= 6
        assert all(0 <= np.array([t[10]], np.uint32).view(np.float32)[0] < 360 for t in group)
    # octaves smaller than the window (4 x 12, 2 x 6 are under 3 rows of candidates) still orient
    assert {t[0] for t in got} >= {0, 1, 2, 3}
    rec = refined_from(records_from_set(want("tie", ODD)[0]))
    got, why = np_orient(tie_pyramid(ODD), H, W, S, O, rec, formula_tables(S))
    assert 0 < why.count("nonfinite") < len(rec) and why.count("ok") > 0


def test_as_multiset_round_trip():
    dt = np.dtype({"names": ["octave", "scale", "kind", "row", "col", "value", "dscale", "drow", "dcol", "interp", "angle",
                             "peak", "bin", "peaks"],
                   "formats": [np.uint16, np.uint8, np.int8, np.int32, np.int32] + [np.float32] * 7 + [np.uint32] * 2,
                   "offsets": [0, 2, 3, 4, 8, 12, 16, 20, 24, 28, 32, 36, 40, 44], "itemsize": 48})
    D = gradient_pyramid(GS, GROWS, GCOLS, 2, -1, 1)
    got, _ = np_orient(D.ravel(), GROWS, GCOLS, GS, 1, refined_records([(2, 9, 9), (3, 4, 30)], kind=-1), formula_tables(GS))
    a = np.zeros(len(got), dt)
    for i, t in enumerate(got):
        for f, v in zip(dt.names[:5], t[:5]):
            a[f][i] = v
        for f, v in zip(dt.names[5:12], t[5:12]):
            a[f][i:i + 1].view(np.uint32)[0] = v
        a["bin"][i], a["peaks"][i] = t[12], t[13]
    assert as_multiset(a) == got and [t[2] for t in got] == [-1, -1]
