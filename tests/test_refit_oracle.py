"""The numpy oracle of the refit rule (tests/refit_oracle.py) checked on its own, without a GPU: its
candidate agrees with an independent least-squares solve to one float32 ulp, does not depend on the
order of the inlier list, reproduces four exact correspondences to the quantisation step, is closer to
a planted map than the RANSAC winner, reports the documented status for degenerate lists, and accepts
and rejects as the rule says."""
import numpy as np
import pytest

from match_oracle import MATCH_DT
from ransac_cases import TIE, collinear_list
from ransac_oracle import F, NONE, PLANTED, matrix, none_record, np_ransac, planted_list
from refit_cases import EXTREME, NOISY, POLLUTED, SKIPPED, TOO_FEW_USED, exact_list, planted_points
from refit_oracle import (ACCEPTED, DEG_Q, DEG_T, FEWER, NO_MODEL, PIVOT, REFIT_DT, TOO_FEW, candidate, count, moments, np_refit,
                          quantise, scale, to_double, transfer_rms)

D = np.float64


def test_record_layout():
    assert REFIT_DT.itemsize == 96
    assert [REFIT_DT.fields[n][1] for n in REFIT_DT.names] == [0, 4, 8, 12, 16, 20, 24, 28, 32, 36, 52, 88]


def test_integer_steps():
    L = np.zeros(3, MATCH_DT)
    L["qx"], L["qy"], L["tx"], L["ty"] = (1.5, -0.001953125, 16383.99), (0.0, -1.0, np.nan), (2.0, 3.0, 4.0), (1e-40, 16384.0, 5.0)
    q, skipped = quantise(L)
    assert q == [(384, 0, 512, 0)] and skipped == 2  # rint to even: -0.5 -> -0; a denormal -> 0; 16384 and NaN are skipped
    assert (-7) // 2 == -4  # the origin's floor division
    assert scale(0, 4) == 0 and scale(3, 4) == 0 and scale(4, 4) == 1 and scale(15, 4) == 1 and scale(16, 4) == 2
    assert to_double(-(1 << 100) - 1, 4) == -D(2.0) ** 96 and to_double((1 << 64) + (1 << 11) + 1, 0) == D(2.0) ** 64 + 4096
    mu = moments([(1, 2, 3, 4), (-1, -2, -3, -4)], (0, 0, 0, 0))
    assert mu[0] == [2, 0, 0, 50] and mu[3] == [2, 0, 0, 50] and mu[4][1] == 0 and mu[1][1] == 6 and mu[5][3] == 200


def lstsq_candidate(L):
    """The same normalised system solved by numpy.linalg.lstsq in float64 and denormalised in plain
    matrix arithmetic: an independent solve of what steps 5 and 6 compute."""
    q, _ = quantise(L)
    cand = candidate(L)
    o, kq, kt = cand["origin"], cand["kq"], cand["kt"]
    c = np.array(q, D) - np.array(o, D)
    x, y, X, Y = c[:, 0] * 2.0 ** -kq, c[:, 1] * 2.0 ** -kq, c[:, 2] * 2.0 ** -kt, c[:, 3] * 2.0 ** -kt
    one, zero = np.ones_like(x), np.zeros_like(x)
    A = np.concatenate([np.stack([x, y, one, zero, zero, zero, -X * x, -X * y], axis=1),
                        np.stack([zero, zero, zero, x, y, one, -Y * x, -Y * y], axis=1)])
    g = np.linalg.lstsq(A, np.concatenate([X, Y]), rcond=None)[0]
    Tq = np.array([[256.0 * 2.0 ** -kq, 0, -o[0] * 2.0 ** -kq], [0, 256.0 * 2.0 ** -kq, -o[1] * 2.0 ** -kq], [0, 0, 1]])
    Tt_inv = np.array([[2.0 ** kt / 256.0, 0, o[2] / 256.0], [0, 2.0 ** kt / 256.0, o[3] / 256.0], [0, 0, 1]])
    G = Tt_inv @ np.append(g, 1.0).reshape(3, 3) @ Tq
    _, e = np.frexp(np.abs(G).max())
    return cand, np.ldexp(G, -e).ravel(), np.linalg.cond(A.T @ A)


def test_against_an_independent_solve():
    """Every entry within 2^-24, one float32 ulp of the [0.5, 1) binade the largest entry lies in: the
    solve's own error is around 1e-13, so the bound is the final float32 rounding plus margin."""
    rng = np.random.default_rng(3)
    worst, conds = 0.0, []
    sizes = [4, 5, 6, 8, 13] + [int(v) for v in rng.integers(14, 2001, 35)]
    for k, n in enumerate(sizes):
        L = planted_list(n, n, 500 + k, noise=float(rng.uniform(0.0, 2.0)))[0]
        cand, want, cond = lstsq_candidate(L)
        assert cand["status"] == 0 and cand["used"] == n, (n, cand)
        err = float(np.abs(cand["h"].astype(D) - want).max())
        worst, conds = max(worst, err), conds + [cond]
        assert err <= 2.0 ** -24, (n, err * 2.0 ** 24)
    print(f"{len(sizes)} lists: worst |candidate - lstsq| = {worst * 2.0 ** 24:.3f} ulp, cond(N) {min(conds):.3g} .. {max(conds):.3g}")


def test_a_permuted_list_gives_the_identical_record():
    M = NOISY(400)
    _, model, L = np_ransac(M, 128, 0)
    want = np_refit(M, model, L, 2, 3.0)
    rng = np.random.default_rng(4)
    for _ in range(3):
        got = np_refit(M, model, L[rng.permutation(len(L))], 2, 3.0)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got, want))
    assert int(want[2]["accepted"]) >= 1


def test_four_exact_correspondences_to_the_quantisation_step():
    """The transfer error on the four points is gated against 1/128 px, twice the 1/256 px step."""
    rng = np.random.default_rng(5)
    worst = 0.0
    for _ in range(20):
        q = rng.uniform((0.0, 0.0), (640.0, 480.0), (4, 2))
        p = np.concatenate([q, np.ones((4, 1))], axis=1) @ PLANTED.T
        L = np.zeros(4, MATCH_DT)
        L["qx"], L["qy"] = q.T
        L["tx"], L["ty"] = (p[:, :2] / p[:, 2:]).T
        cand = candidate(L)
        assert cand["status"] == 0
        pts = np.stack([L["qx"], L["qy"]], axis=1).astype(D), np.stack([L["tx"], L["ty"]], axis=1).astype(D)
        for a, b in zip(*pts):
            worst = max(worst, transfer_rms(cand["h"], a[None], b[None]))
    print(f"four exact correspondences: worst transfer error {worst:.5f} px = {worst * 256:.3f} steps")
    assert worst < 1.0 / 128


@pytest.mark.parametrize("n,sigma", [(60, 0.5), (400, 0.5), (2000, 0.5), (400, 0.1), (400, 1.0)])
def test_the_refit_is_closer_to_the_planted_map_than_the_winner(n, sigma):
    M = NOISY(n, sigma)
    _, model, L = np_ransac(M, 256, 0)
    refit, L2, rec = np_refit(M, model, L, 1, 3.0)
    q, t = planted_points()
    before, after = transfer_rms(model["h"], q, t), transfer_rms(refit["h"], q, t)
    print(f"n = {n}, sigma = {sigma}: RMS to the planted map {before:.3f} px -> {after:.3f} px, inliers {len(L)} -> {len(L2)}")
    assert int(rec["status"]) == ACCEPTED and after < before
    assert int(refit["hypothesis"]) == int(model["hypothesis"]) and (refit["sample"] == model["sample"]).all()
    assert int(refit["inliers"]) == len(L2) == int(rec["count_after"]) and int(rec["count_before"]) == len(L)


def test_degenerate_lists_give_the_documented_status():
    rng = np.random.default_rng(6)
    line = collinear_list(64)[::2]  # every query point on y = 2x + 1
    assert candidate(line)["status"] == PIVOT
    assert candidate(np.repeat(exact_list(3), 5))["status"] == PIVOT  # 15 records, three distinct points
    assert candidate(np.repeat(exact_list(4), 5))["status"] == 0  # four distinct points are enough
    for n in range(4):
        c = candidate(exact_list(8)[:n])
        assert c["status"] == TOO_FEW and c["used"] == n and not c["h"].any() and c["origin"] == (0, 0, 0, 0)
    bad = exact_list(8).copy()
    bad["qx"][:3], bad["ty"][3:5] = np.nan, np.inf
    c = candidate(bad)
    assert c["status"] == TOO_FEW and (c["used"], c["skipped"]) == (3, 5)
    R = np.frombuffer(rng.bytes(32 * 500), MATCH_DT)
    c = candidate(R)  # whatever it is, it does not raise
    assert c["used"] + c["skipped"] == 500 and 0 < c["used"] < 500 and c["status"] in (0, PIVOT, 4)
    M, H, seed, t = EXTREME()
    c = candidate(M)
    assert c["status"] == 0 and c["used"] == 300 and c["kq"] == c["kt"] == 23 and np.isfinite(c["h"]).all()
    assert transfer_rms(c["h"], np.stack([M["qx"], M["qy"]], axis=1), np.stack([M["tx"], M["ty"]], axis=1)) < 1.0 / 128
    M, H, seed, t = SKIPPED()
    c = candidate(M)
    assert c["skipped"] > 50 and c["used"] + c["skipped"] == len(M)


def test_the_gpu_cases_are_what_they_claim():
    M, H, seed, t = TOO_FEW_USED()
    _, model, L = np_ransac(M, H, seed, t)
    assert len(L) == 6
    refit, L2, rec = np_refit(M, model, L, 3, t)
    assert int(rec["status"]) == TOO_FEW and (int(rec["used"]), int(rec["skipped"]), int(rec["accepted"])) == (3, 3, 0)
    assert refit.tobytes() == model.tobytes() and L2.tobytes() == L.tobytes() and int(rec["count_before"]) == int(rec["count_after"]) == 6
    M, H, seed, t = SKIPPED()
    _, model, L = np_ransac(M, H, seed, t)
    refit, L2, rec = np_refit(M, model, L, 1, 3.0)
    assert int(rec["skipped"]) >= 1 and int(rec["used"]) >= 100 and int(rec["status"]) in (ACCEPTED, FEWER)
    M, H, seed, t = EXTREME()
    _, model, L = np_ransac(M, H, seed, t)
    assert len(L) == 300
    assert int(np_refit(M, model, L, 1, t)[2]["status"]) == ACCEPTED
    for k in (4, 5, 63, 64, 65, 255, 256, 257):
        for extra in (0, 40)[:1 + (k > 5)]:  # 256 hypotheses find five of 45 too rarely
            M = exact_list(k, extra)
            _, model, L = np_ransac(M, 256, 0)
            assert len(L) == k, (k, extra, len(L))


def test_acceptance_on_equality_and_rejection():
    M, H, seed = TIE()
    _, model, L = np_ransac(M, H, seed)
    refit, L2, rec = np_refit(M, model, L, 1, 3.0)
    assert int(rec["status"]) == ACCEPTED and int(rec["count_before"]) == int(rec["count_after"]) == 150  # c_new = c_cur
    assert refit["h"].tobytes() != model["h"].tobytes() and L2.tobytes() == L.tobytes()
    M, H, seed, t = POLLUTED()
    _, model, L = np_ransac(M, H, seed, t)
    refit, L2, rec = np_refit(M, model, L, 8, t)
    c_new, _ = count(rec["h"], M, t)
    assert int(rec["status"]) == FEWER and 4 <= c_new < int(rec["count_before"]) and int(rec["accepted"]) == 0
    assert refit.tobytes() == model.tobytes() and L2.tobytes() == L.tobytes()  # everything is left as it was
    assert int(rec["count_after"]) == int(model["inliers"]) and int(rec["rounds"]) == 8
    # the same list under a tighter refit threshold: the candidate is judged under the refit's threshold
    refit, L2, rec = np_refit(M, model, L, 2, 3.0)
    assert int(rec["accepted"]) >= 1 and int(rec["count_before"]) < int(model["inliers"])


def test_no_model_does_nothing():
    M = exact_list(8)
    model, L, rec = np_refit(M, none_record(8), M[:0], 3, 3.0)
    assert int(rec["status"]) == NO_MODEL and int(rec["rounds"]) == 3 and not rec["h"].any()
    assert int(model["hypothesis"]) == NONE and matrix(model) is None and len(L) == 0
    assert all(int(rec[f]) == 0 for f in ("accepted", "used", "skipped", "count_before", "count_after", "kq", "kt"))
    assert DEG_Q == (0, 1, 1, 2, 2, 2) and DEG_T == (0, 1, 1, 2) and F(1).dtype == np.float32
