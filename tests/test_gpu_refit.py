"""On-device least-squares refit of the RANSAC homography (gdp_refit_homography) against the literal
oracle of tests/refit_oracle.py.  The moments are exact integers, the solve is separately rounded
float64, the scoring separately rounded float32 and the counts are integer sums, so the result is
exact: after a fit and a refit the model record, the refit record (the candidate's h[9] included), the
sorted inlier list and the counter equal the oracle's byte for byte.  The synthetic cases run on a
40 x 56, S = 2, two-octave context with the caller's lists (gdp_ransac_set_input); the downstream,
state and example cases run the chain on tiny frames."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from guided_oracle import np_guided
from ransac_cases import TIE, collinear_list
from ransac_oracle import NONE, matrix, np_ransac
from refit_cases import EXTREME, NOISY, POLLUTED, SKIPPED, TOO_FEW_USED, exact_list
from refit_oracle import ACCEPTED, FEWER, NO_MODEL, TOO_FEW, np_refit
from test_gpu_match import chain, raw_described
from test_gpu_ransac import CAPACITY, raw_matches, small_context
from test_gpu_warp import QH, QW, TH, TW, assert_same, run_chain, scene
from warp_oracle import np_warp_model

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PER_BLOCK, MAX_BLOCKS = 2048, 1024  # the sweeps over L and M: min(1024, ceil(capacity / 2048)) blocks of 256 threads


def results(ctx):
    got = ctx.inliers()
    assert got.found == ctx.inlier_count() == len(got)
    return ctx.homography(), got, ctx.refit_record()


def assert_equal(pkg, got, want, what):
    (model, inliers, rec), (want_model, want_inliers, want_rec) = got, want
    assert model.dtype == pkg.HOMOGRAPHY_DTYPE and inliers.dtype == pkg.MATCH_DTYPE and rec.dtype == pkg.REFIT_DTYPE
    assert rec.tobytes() == want_rec.tobytes(), (what, rec, want_rec)
    assert model.tobytes() == want_model.tobytes(), (what, model, want_model)
    assert inliers.tobytes() == want_inliers.tobytes(), (what, len(inliers), len(want_inliers))


def assert_refit(pkg, ctx, M, H, seed=0, fit_threshold=3.0, rounds=1, threshold=3.0, min_inliers=4, what=None):
    """One fit and one refit of the caller's list M, byte for byte; returns the oracle's records."""
    ctx.set_ransac_input(M)
    ctx.fit_homography(H, seed, fit_threshold, min_inliers)
    ctx.refit_homography(rounds, threshold)  # the same stream, no host read in between
    _, model, L = np_ransac(M, H, seed, fit_threshold, min_inliers)
    want = np_refit(M, model, L, rounds, threshold)
    assert_equal(pkg, results(ctx), want, what)
    return (model, L) + want


# ---------------------------------------------------------------------------------------------
# 1. list sizes: |L| and n at the wave and block seams, and a list of several grid-stride sweeps
# ---------------------------------------------------------------------------------------------
def test_list_sizes_at_every_seam(pkg):
    seen_l, seen_n, accepted = set(), set(), 0
    with small_context(pkg) as ctx:
        assert ctx.refit_record().tobytes() == bytes(96)  # all 0 before any refit
        for k in (4, 5, 63, 64, 65, 255, 256, 257):
            for extra in (0, 40)[:1 + (k > 5)]:
                _, L, model, _, rec = assert_refit(pkg, ctx, exact_list(k, extra), 256, what=("exact", k, extra))
                seen_l.add(len(L))
                seen_n.add(k + extra)
                accepted += int(rec["status"]) == ACCEPTED
        for n in (0, 3, 4, 5, 63, 64, 65, 255, 256, 257, CAPACITY):
            _, L, model, _, rec = assert_refit(pkg, ctx, NOISY(n), 256, rounds=2, what=("noisy", n))
            seen_l.add(len(L))
            seen_n.add(n)
            accepted += int(rec["accepted"])
    print("inlier lists:", sorted(seen_l), "accepted rounds:", accepted)
    assert {0, 4, 5, 63, 64, 65, 255, 256, 257} <= seen_l and {0, 3, 4, 5, 63, 64, 65, 255, 256, 257} <= seen_n and accepted >= 20


def test_a_list_longer_than_one_sweep(pkg):
    capacity = 5000
    with small_context(pkg, capacity, 128) as ctx:
        threads = 256 * min(MAX_BLOCKS, -(-ctx.ransac_layout()[0] // PER_BLOCK))
        assert threads == 768
        _, L, _, L2, rec = assert_refit(pkg, ctx, NOISY(capacity), 128, rounds=2, what="long")
        assert len(L) > 4 * threads and int(rec["accepted"]) >= 1 and len(L2) >= len(L)


# ---------------------------------------------------------------------------------------------
# 2. values
# ---------------------------------------------------------------------------------------------
def test_extreme_coordinates_reach_the_top_limbs(pkg):
    M, H, seed, t = EXTREME()
    with small_context(pkg) as ctx:
        _, L, model, _, rec = assert_refit(pkg, ctx, M, H, seed, t, what="extreme")
    assert len(L) == 300 and int(rec["status"]) == ACCEPTED and int(rec["kq"]) == int(rec["kt"]) == 23


def test_skipped_records(pkg):
    M, H, seed, t = SKIPPED()
    with small_context(pkg) as ctx:
        _, L, _, _, rec = assert_refit(pkg, ctx, M, H, seed, t, what="skipped")
        assert int(rec["skipped"]) >= 1 and int(rec["used"]) + int(rec["skipped"]) == len(L)
        M, H, seed, t = TOO_FEW_USED()
        model, L, refit, L2, rec = assert_refit(pkg, ctx, M, H, seed, t, rounds=3, what="too few used")
        assert int(rec["status"]) == TOO_FEW and int(rec["used"]) == 3 and refit.tobytes() == model.tobytes() and len(L2) == 6


@pytest.mark.parametrize("rounds", [1, 2, 8])
def test_rounds(pkg, rounds):
    with small_context(pkg) as ctx:
        _, _, _, _, rec = assert_refit(pkg, ctx, NOISY(400, 1.0), 256, rounds=rounds, what=rounds)
        assert int(rec["rounds"]) == rounds and 1 <= int(rec["accepted"]) <= rounds
        assert_refit(pkg, ctx, NOISY(300, 0.5, 1), 64, 1, rounds=rounds, what=(rounds, "again"))  # the state of the first is gone


def test_thresholds(pkg):
    M = NOISY(400, 1.0)
    with small_context(pkg) as ctx:
        for fit_threshold, threshold in ((3.0, 1.0), (1.0, 3.0), (3.0, 0.0), (0.0, 0.0), (3.0, -0.0), (6.0, 0.25)):
            assert_refit(pkg, ctx, M, 256, 0, fit_threshold, 2, threshold, what=(fit_threshold, threshold))
        for threshold in (0.0, 3.0):  # integer coordinates: e == 0 does occur
            assert_refit(pkg, ctx, collinear_list(64), 256, 0, threshold, 2, threshold, what=("collinear", threshold))


def test_a_rejected_round_and_one_accepted_on_equality(pkg):
    with small_context(pkg) as ctx:
        M, H, seed, t = POLLUTED()
        model, L, refit, L2, rec = assert_refit(pkg, ctx, M, H, seed, t, 8, t, what="rejected")
        assert int(rec["status"]) == FEWER and int(rec["accepted"]) == 0 and rec["h"].any()
        assert refit.tobytes() == model.tobytes() and L2.tobytes() == L.tobytes()
        M, H, seed = TIE()
        _, _, _, _, rec = assert_refit(pkg, ctx, M, H, seed, what="equality")
        assert int(rec["status"]) == ACCEPTED and int(rec["count_before"]) == int(rec["count_after"]) == 150


def test_no_model_stays_none(pkg):
    M = NOISY(100)
    with small_context(pkg) as ctx:
        _, _, model, L, rec = assert_refit(pkg, ctx, M, 128, min_inliers=1000, rounds=3, what="none")
        assert matrix(model) is None and len(L) == 0 and int(rec["status"]) == NO_MODEL and int(rec["rounds"]) == 3
        assert int(ctx.homography()["hypothesis"]) == NONE and ctx.inlier_count() == 0
        assert_refit(pkg, ctx, M[:0], 16, what="empty")  # an empty list is a list


# ---------------------------------------------------------------------------------------------
# 3. refusals; a second fit after a refit
# ---------------------------------------------------------------------------------------------
def test_refusals_leave_the_previous_result(pkg):
    with small_context(pkg) as ctx:
        for kw, word in (({"rounds": 0}, "rounds"), ({"rounds": 9}, "rounds")):  # before any refit: nothing is allocated either
            with pytest.raises(pkg.GdpError) as e:
                ctx.refit_homography(**kw)
            assert e.value.status == 1 and word in str(e.value) and ctx.refit_record().tobytes() == bytes(96)
        L, view = pkg.lib(), ctypes.c_void_p()
        assert L.gdp_device_refit(ctx._ransac, ctypes.byref(view)) == 3 and view.value is None  # GDP_ERR_STATE before the first refit
        assert_refit(pkg, ctx, NOISY(200), 128, rounds=2, what="before")
        before = tuple(r.tobytes() for r in results(ctx))
        assert L.gdp_device_refit(ctx._ransac, ctypes.byref(view)) == 0 and view.value
        hip, raw = ctypes.CDLL("libamdhip64.so"), np.zeros(96, np.uint8)
        hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
        assert hip.hipMemcpy(raw.ctypes.data, view, raw.nbytes, 2) == 0 and raw.tobytes() == before[2]  # the zero-copy view is the record
        for kw, word in (({"rounds": 0}, "rounds"), ({"rounds": 9}, "rounds"), ({"threshold": -1.0}, "threshold"),
                         ({"threshold": float("nan")}, "threshold"), ({"threshold": float("inf")}, "threshold")):
            with pytest.raises(pkg.GdpError) as e:
                ctx.refit_homography(**kw)
            assert e.value.status == 1 and word in str(e.value)
            assert tuple(r.tobytes() for r in results(ctx)) == before


def test_a_second_fit_after_a_refit_gives_what_it_gives_without_one(pkg):
    M = NOISY(300, 1.0)
    with small_context(pkg) as ctx:
        ctx.set_ransac_input(M)
        ctx.fit_homography(128, 3)
        plain = (ctx.hypotheses().tobytes(), ctx.homography().tobytes(), ctx.inliers().tobytes())
        ctx.refit_homography(2)
        refit, _, rec = results(ctx)
        assert int(rec["accepted"]) >= 1 and refit.tobytes() != plain[1]
        ctx.fit_homography(128, 3)
        assert (ctx.hypotheses().tobytes(), ctx.homography().tobytes(), ctx.inliers().tobytes()) == plain
        assert ctx.refit_record().tobytes() == rec.tobytes()  # the record stays that of the last refit


# ---------------------------------------------------------------------------------------------
# 4. downstream: the warp and the guided match consume the refit model on the same stream
# ---------------------------------------------------------------------------------------------
def test_warp_and_guided_match_consume_the_refit_model(pkg, oracle):
    qimg, timg = scene(oracle)
    with pkg.PyramidContext(QH, QW, S=2, octaves=2) as q, pkg.PyramidContext(TH, TW, S=2, octaves=2) as t:
        run_chain(q, t, qimg, timg)
        q.match_descriptors(t, ratio=0.8)  # nearly every match is an inlier, so any device order of the list gives an accepted refit
        q.fit_homography(512, 3, 2.0)
        q.refit_homography(2, 2.0)
        q.warp_image(0, fill=-1)
        q.guided_match(3.0, ratio=0.8, unique=True)  # the same stream, no synchronisation and no host read above
        M = raw_matches(pkg, q)
        _, model, L = np_ransac(M, 512, 3, 2.0)
        want = np_refit(M, model, L, 2, 2.0)
        assert len(M) >= 4 and matrix(model) is not None and int(want[2]["accepted"]) >= 1  # the test cannot pass empty
        assert want[0]["h"].tobytes() != model["h"].tobytes()
        assert_equal(pkg, results(q), want, "pipeline")
        assert_same(pkg, q, np_warp_model(want[0], 0, qimg, timg, -1), "warp under the refit model")
        guided = np_guided(raw_described(pkg, q, 0), raw_described(pkg, t, 0), want[0]["h"], 3.0, 0.8)
        assert q.guided_matches().tobytes() == guided.tobytes() and len(guided) >= 16


# ---------------------------------------------------------------------------------------------
# 5. state: the refit writes nothing of a context
# ---------------------------------------------------------------------------------------------
def test_the_context_is_left_as_it_was(pkg, oracle):
    n, S = 64, 2
    with pkg.PyramidContext(n, n, S=S) as ctx:
        ctx.set_input(oracle.lcg_image(n, n, 12345))
        ctx.build()
        ctx.build()
        assert ctx.tuning()["zeros_clean"] == 1
        chain(ctx)
        ctx.match_descriptors(ratio=0.0)
        state = lambda: (ctx.checksum(0), ctx.keypoints(0).tobytes(), ctx.refined_keypoints(0).tobytes(),  # noqa: E731
                         ctx.oriented_keypoints(0).tobytes(), ctx.described_keypoints(0).tobytes(), ctx.matches().tobytes(),
                         raw_matches(pkg, ctx).tobytes(), ctx.pyramid(0).tobytes())
        before = state()
        ctx.fit_homography(256, 2)
        ctx.refit_homography(2)
        M = raw_matches(pkg, ctx)
        _, model, L = np_ransac(M, 256, 2)
        assert_equal(pkg, results(ctx), np_refit(M, model, L, 2, 3.0), "state")
        assert ctx.tuning()["zeros_clean"] == 1  # the next build is still the steady-state one
        assert state() == before and len(before[5]) > 0 and len(M) >= 4
        ctx.build()
        assert ctx.tuning()["zeros_clean"] == 1 and ctx.checksum(0) == before[0]


# ---------------------------------------------------------------------------------------------
# 6. the C++ example, executed
# ---------------------------------------------------------------------------------------------
def test_cpp_example_gives_the_python_paths_records(pkg, oracle):
    """Two 64 x 64 LCG images, the second moved 16 columns to the right.  The example fits and refits
    the matches sorted by their coordinates, which do not depend on the described lists' device order,
    so the records' bits must be those of the Python path on the same sorted list."""
    exe = os.path.join(REPO, "examples", "refit_hip")
    subprocess.run(["make", "-s", "-C", os.path.join(REPO, "examples"), "refit_hip"], check=True)  # never a stale binary
    n, S, seed, shift = 64, 2, 12345, 16
    out = subprocess.run([exe, str(n), str(S), f"lcg:{seed}", str(shift), "0.5", "10", "0.8", "256", "7", "3.0", "2", "2.0"], check=True,
                         timeout=120, capture_output=True, text=True).stdout
    print(out)
    heads = re.findall(r"^(fit|refit): (\d+) inliers of (\d+) matches\nhypothesis (\d+) inliers (\d+) matches (\d+)", out, re.M)
    bits = [int(word, 16) for row in re.findall(r"^h (\w{8}) (\w{8}) (\w{8})", out, re.M) for word in row]
    record = [int(word, 16) for word in re.search(r"^record((?: \w{8}){24})$", out, re.M).group(1).split()]
    assert [h[0] for h in heads] == ["fit", "refit"] and len(bits) == 18
    img = oracle.lcg_image(n, n, seed)
    with pkg.PyramidContext(n, n, S=S) as a, pkg.PyramidContext(n, n, S=S) as b:
        for ctx, image in ((a, img), (b, np.roll(img, shift, axis=1))):
            ctx.set_input(np.ascontiguousarray(image))
            ctx.build_gaussian()
            ctx.detect_extrema()
            ctx.refine_keypoints(0.5, 10.0)
            ctx.orient_keypoints()
            ctx.describe_keypoints()
        b.sync()
        a.match_descriptors(b, ratio=0.8, mutual=True)
        M = np.asarray(a.matches())
        M = M[np.lexsort((M["second"], M["distance"], M["ty"], M["tx"], M["qy"], M["qx"]))]
        model, L, refit, L2, rec = assert_refit(pkg, a, M, 256, 7, 3.0, 2, 2.0, what="example")
    assert len(M) >= 4
    assert [int(x) for x in heads[0][1:]] == [len(L), len(M), int(model["hypothesis"]), int(model["inliers"]), int(model["matches"])]
    assert [int(x) for x in heads[1][1:]] == [len(L2), len(M), int(refit["hypothesis"]), int(refit["inliers"]), int(refit["matches"])]
    assert bits == [int(w) for w in model["h"].view(np.uint32)] + [int(w) for w in refit["h"].view(np.uint32)]
    assert record == [int(w) for w in np.frombuffer(rec.tobytes(), np.uint32)]
