"""The numpy oracle of the RANSAC homography rule (tests/ransac_oracle.py) checked on its own, without
a GPU: its float32 steps stay float32, its sampler is the integer rule, it recovers planted
homographies, its four-point fit agrees with an SVD solution, and the conditions the GPU cases rely
on hold."""
import numpy as np
import pytest

from match_oracle import MATCH_DT
from ransac_oracle import F, HOMOGRAPHY_DT, NONE, PLANTED, fit, inlier_mask, matrix, mix, np_ransac, planted_list, sample, score
from ransac_cases import NO_VALID, TIE, collinear_list


def test_record_layout():
    assert HOMOGRAPHY_DT.itemsize == 64
    assert [HOMOGRAPHY_DT.fields[n][1] for n in HOMOGRAPHY_DT.names] == [0, 36, 40, 44, 48]


def test_float32_steps_stay_float32():
    M, _ = planted_list(50, 40, 1)
    assert all(M[f].dtype == F for f in ("qx", "qy", "tx", "ty"))
    hyp = fit(M, 8, 0)
    assert hyp["h"].dtype == F
    tt = F(3.0) * F(3.0)
    assert type(tt) is F
    h = [np.ascontiguousarray(hyp["h"][:, k])[:, None] for k in range(9)]
    mask = inlier_mask(h, M["qx"][None, :], M["qy"][None, :], M["tx"][None, :], M["ty"][None, :], tt)  # asserts every dtype inside
    assert mask.dtype == bool and mask.shape == (8, 50)
    # a float64 slipping in would be caught: the same call with a float64 threshold fails its own assert
    with pytest.raises(AssertionError):
        inlier_mask(h, M["qx"][None, :], M["qy"][None, :], M["tx"][None, :], M["ty"][None, :], np.float64(9.0))


def _mix_int(x):
    x ^= x >> 16
    x = (x * 0x7FEB352D) % 2 ** 32
    x ^= x >> 15
    x = (x * 0x846CA68B) % 2 ** 32
    x ^= x >> 16
    return x


@pytest.mark.parametrize("n,H,seed", [(0, 5, 0), (3, 5, 1), (4, 64, 7), (5, 100, 0xFFFFFFFF), (1100, 300, 0x9E3779B9), (384867, 50, 12345)])
def test_sampler_is_the_integer_rule(n, H, seed):
    idx, valid = sample(n, H, seed)
    assert idx.dtype == np.uint32 and idx.shape == (H, 4)
    for h in range(H):
        want = [(_mix_int((seed + 0x9E3779B9 * (4 * h + k + 1)) % 2 ** 32) * n) >> 32 for k in range(4)]
        assert [int(v) for v in idx[h]] == want
        assert bool(valid[h]) == (n >= 4 and len(set(want)) == 4)
    assert int(mix(np.array([0]))[0]) == 0 and int(mix(np.array([1]))[0]) == _mix_int(1)


@pytest.mark.parametrize("n,inliers,H,seed", [(40, 40, 64, 0), (200, 100, 256, 1), (1100, 700, 256, 2), (4313, 2200, 1024, 3), (9, 8, 64, 4)])
def test_planted_inliers_are_recovered(n, inliers, H, seed):
    M, planted = planted_list(n, inliers, seed)
    hyp, model, got = np_ransac(M, H, seed, 3.0)
    assert matrix(model) is not None and int(model["inliers"]) == inliers == len(got)
    assert got.tobytes() == M[planted].tobytes()  # the list is in `query` order already
    assert int(hyp["inliers"].max()) == inliers and int(model["hypothesis"]) == int(np.argmax(hyp["inliers"]))
    # the model is the planted transform up to scale, loosely (noise of 0.1 pixel on four points)
    G = matrix(model).astype(np.float64)
    assert np.abs(G / G[2, 2] - PLANTED / PLANTED[2, 2])[:2, :2].max() < 0.05


def _dlt(q, t):
    rows = []
    for (x, y), (X, Y) in zip(q, t):
        rows.append([-x, -y, -1, 0, 0, 0, X * x, X * y, X])
        rows.append([0, 0, 0, -x, -y, -1, Y * x, Y * y, Y])
    return np.linalg.svd(np.array(rows, np.float64))[2][-1].reshape(3, 3)


def test_four_point_fit_agrees_with_an_svd_dlt():
    """An all-inlier list without noise: every valid hypothesis is the exact homography of its four
    points, which an independent SVD null vector gives as well.  Both scaled to max |h| = 1 and to the
    same sign.  The rule's result is rounded to float32 (relative 2^-24 = 6e-8 per entry); the rest is
    the conditioning of four random points.  Measured here over the 200 hypotheses: the largest entry
    difference over the 196 valid ones is 3.5e-7 (median 1.2e-8); the bound is 4e-6, eleven times the
    worst seen."""
    M, _ = planted_list(300, 300, 5, noise=0.0)
    hyp = fit(M, 200, 9)
    worst, diffs = 0.0, []
    for r in hyp:
        if not r["h"].any():
            continue
        s = M[r["sample"]]
        D = _dlt(np.stack([s["qx"], s["qy"]], 1).astype(np.float64), np.stack([s["tx"], s["ty"]], 1).astype(np.float64))
        G = r["h"].astype(np.float64).reshape(3, 3)
        k = np.unravel_index(np.argmax(np.abs(G)), G.shape)
        G, D = G / G[k], D / D[k]
        assert np.abs(G).max() == 1.0
        diffs.append(np.abs(G - D).max() / np.abs(D).max())
        worst = max(worst, diffs[-1])
    print(f"{len(diffs)} valid hypotheses: worst {worst:.3g}, median {np.median(diffs):.3g}")
    assert len(diffs) > 150 and worst < 4e-6


def test_normalisation_and_orientation():
    M, _ = planted_list(300, 300, 5)
    hyp = fit(M, 64, 3)
    big = np.abs(hyp["h"]).max(axis=1)
    valid = big > 0
    assert valid.sum() > 50 and ((big[valid] >= 0.5) & (big[valid] <= 1.0)).all()
    for r in hyp[valid]:  # w > 0 at the sample's first query point
        s = M[r["sample"][0]]
        assert (r["h"][6] * s["qx"] + r["h"][7] * s["qy"]) + r["h"][8] > 0
    assert (hyp["hypothesis"] == np.arange(64)).all() and (hyp["matches"] == 300).all() and not hyp["inliers"].any()


def test_the_tie_case_has_two_winning_hypotheses():
    M, H, seed = TIE()
    hyp, model, got = np_ransac(M, H, seed, 3.0)
    best = int(hyp["inliers"].max())
    tied = np.flatnonzero(hyp["inliers"] == best)
    assert len(tied) >= 2 and int(model["hypothesis"]) == int(tied[0]) and len(got) == best >= 4
    assert not np.array_equal(hyp["sample"][tied[0]], hyp["sample"][tied[1]])  # two different samples


def test_the_no_valid_hypothesis_case_has_none():
    M, H, seed = NO_VALID()
    assert len(M) == 4
    _, valid = sample(4, H, seed)
    assert not valid.any()
    hyp, model, got = np_ransac(M, H, seed, 3.0)
    assert not hyp["h"].any() and not hyp["inliers"].any() and len(got) == 0
    assert int(model["hypothesis"]) == NONE and (model["sample"] == NONE).all() and matrix(model) is None and int(model["matches"]) == 4
    _, valid = sample(4, 64, seed)  # with more hypotheses the same seed does find a valid one: the case rests on H
    assert valid.any()


def test_collinear_samples_are_invalid_or_harmless():
    """The collinear case really draws samples with three and with four query points on one line; four
    give lambda = 0 exactly, so an all-zero (invalid) record, and none of them accepts the whole list."""
    M = collinear_list(64)
    hyp, model, got = np_ransac(M, 256, 0, 3.0)
    _, distinct = sample(64, 256, 0)
    on_line = (hyp["sample"] % 2 == 0).sum(axis=1)  # even records lie on the line
    assert (distinct & (on_line == 3)).sum() > 10 and (distinct & (on_line == 4)).sum() > 3
    for r in hyp[distinct & (on_line == 4)]:
        assert not r["h"].any() and r["inliers"] == 0
    degenerate = distinct & (on_line >= 3)
    assert int(hyp["inliers"][degenerate].max()) < 64 == int(hyp["inliers"].max())  # a sound sample gets all: the map is exact


def test_min_inliers_and_threshold_zero():
    M, planted = planted_list(100, 60, 6)
    _, model, got = np_ransac(M, 128, 0, 3.0)
    count = int(model["inliers"])
    assert count == 60
    assert matrix(np_ransac(M, 128, 0, 3.0, count)[1]) is not None
    _, none, empty = np_ransac(M, 128, 0, 3.0, count + 1)
    assert matrix(none) is None and len(empty) == 0 and int(none["inliers"]) == 0
    for low in (0, 1, 3):  # below 4 behaves as 4
        assert np_ransac(M, 128, 0, 3.0, low)[1].tobytes() == model.tobytes()
    hyp0, model0, got0 = np_ransac(M, 128, 0, 0.0)  # e <= 0: only exact fits count
    assert int(hyp0["inliers"].max()) <= 8
    assert score(hyp0, M, 0.0).tolist() == hyp0["inliers"].tolist()


def test_records_of_random_bytes_and_non_finite_coordinates_are_data():
    rng = np.random.default_rng(8)
    M = np.frombuffer(rng.bytes(32 * 300), MATCH_DT).copy()
    hyp, model, got = np_ransac(M, 128, 1, 3.0)
    assert hyp["matches"].tolist() == [300] * 128 and np.isfinite(hyp["h"]).all()
    P, _ = planted_list(100, 80, 9)
    P["qx"][::7], P["ty"][3::11], P["tx"][5::13] = np.nan, np.inf, -np.inf
    hyp, model, got = np_ransac(P, 128, 1, 3.0)
    assert np.isfinite(hyp["h"]).all() and np.isfinite(got["qx"]).all() and np.isfinite(got["ty"]).all() and len(got) > 40
