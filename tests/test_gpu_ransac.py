"""On-device RANSAC homography (gdp_fit_homography) against the literal numpy oracle of
tests/ransac_oracle.py.  The sampler is integer, the fit is separately rounded float64, the scoring
separately rounded float32 and the counts are integer sums, so the result is exact: every comparison
is equality of the downloaded bytes — all H hypothesis records, the model record and the sorted
inlier list — with the oracle's.  The synthetic cases run on a 40 x 56, S = 2, two-octave context with
the caller's lists (gdp_ransac_set_input); the pipeline, state and example cases read the match list
where it lies."""
import ctypes
import functools
import os
import re
import subprocess

import numpy as np
import pytest

from extrema_oracle import ODD, assert_short_downloads, smooth_pyramid
from match_oracle import MATCH_DT
from ransac_cases import NO_VALID, TIE, collinear_list
from ransac_oracle import HOMOGRAPHY_DT, NONE, matrix, np_ransac, planted_list
from test_gpu_match import chain, variant_pyramid

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAPACITY, MAX_H = 1100, 520  # 18 chunks of the match list at most; two full hypothesis blocks and a partial one
SEEDS = (0, 0x9E3779B9)


def small_context(pkg, capacity=CAPACITY, max_hypotheses=MAX_H):
    ctx = pkg.PyramidContext(40, 56, S=2, octaves=2)
    ctx.set_match_capacity(CAPACITY, CAPACITY)
    ctx.set_ransac_capacity(capacity, max_hypotheses)
    return ctx


@functools.lru_cache(maxsize=None)
def planted(n, seed=0):
    M, _ = planted_list(n, (7 * n + 9) // 10, 100 + n + seed)
    M.setflags(write=False)
    return M


def results(ctx):
    got = ctx.inliers()
    assert got.found == ctx.inlier_count() == len(got)
    return ctx.hypotheses(), ctx.homography(), got


def assert_fit(pkg, ctx, M, H, seed=0, threshold=3.0, min_inliers=4, what=None, set_input=True):
    """One fit of the list M (the caller's, or what the device read), byte for byte."""
    if set_input:
        ctx.set_ransac_input(M)
    ctx.fit_homography(H, seed, threshold, min_inliers)
    hyp, model, got = results(ctx)
    want_hyp, want_model, want = np_ransac(M, H, seed, threshold, min_inliers)
    assert hyp.dtype == model.dtype == pkg.HOMOGRAPHY_DTYPE and got.dtype == pkg.MATCH_DTYPE
    assert len(hyp) == H, (what, len(hyp))
    if hyp.tobytes() != want_hyp.tobytes():
        bad = [h for h in range(H) if hyp[h].tobytes() != want_hyp[h].tobytes()]
        raise AssertionError((what, "hypotheses differ", len(bad), hyp[bad[0]], want_hyp[bad[0]]))
    assert model.tobytes() == want_model.tobytes(), (what, model, want_model)
    assert got.tobytes() == want.tobytes(), (what, len(got), len(want))
    assert (matrix(want_model) is None) == (model.matrix is None)
    return want_hyp, want_model, want


# ---------------------------------------------------------------------------------------------
# 1. the caller's lists: every length and every H at the tile, block and chunk seams
# ---------------------------------------------------------------------------------------------
def test_layout_is_what_the_test_mirrors(pkg):
    with small_context(pkg) as ctx:
        assert ctx.ransac_layout() == (CAPACITY, MAX_H, 64, 256)
    with small_context(pkg, 0, 0) as ctx:  # 0: the match object's query capacity, and 4,096 hypotheses
        assert ctx.ransac_layout()[:2] == (CAPACITY, 4096)
    with small_context(pkg, 16, 65537) as ctx:
        with pytest.raises(pkg.GdpError) as e:
            ctx.ransac_layout()
        assert e.value.status == 1 and "65,536" in str(e.value)


def test_callers_lists_at_every_seam(pkg):
    models = 0
    with small_context(pkg) as ctx:
        _, most, tile, block = ctx.ransac_layout()
        lengths = (0, 1, 3, 4, 5, 63, 64, 65, tile - 1, tile, tile + 1, 2 * tile + 1, 3 * tile, CAPACITY - 1, CAPACITY)
        for n in sorted(set(lengths)):
            for H in sorted({1, 63, 64, 65, block - 1, block, block + 1, most}):
                for seed in SEEDS:
                    _, model, _ = assert_fit(pkg, ctx, planted(n), H, seed, what=(n, H, seed))
                    models += matrix(model) is not None
    print("fits with a model:", models)
    assert models > 100  # the comparisons are not all of "none"


def test_the_default_max_hypotheses(pkg):
    with small_context(pkg, 300, 0) as ctx:
        _, model, got = assert_fit(pkg, ctx, planted(300), 4096, 5)
        assert len(got) == 210 and matrix(model) is not None
    with small_context(pkg, 300, 65536) as ctx:
        assert_fit(pkg, ctx, planted(129), 65536, 6)


# ---------------------------------------------------------------------------------------------
# 2. values
# ---------------------------------------------------------------------------------------------
def test_a_tie_goes_to_the_lowest_index(pkg):
    M, H, seed = TIE()
    with small_context(pkg) as ctx:
        hyp, model, got = assert_fit(pkg, ctx, M, H, seed)
    tied = np.flatnonzero(hyp["inliers"] == hyp["inliers"].max())
    assert len(tied) >= 2 and int(model["hypothesis"]) == int(tied[0]) and len(got) == 150


def test_no_valid_hypothesis_gives_no_model(pkg):
    M, H, seed = NO_VALID()
    with small_context(pkg) as ctx:
        hyp, model, got = assert_fit(pkg, ctx, M, H, seed)
        assert not hyp["h"].any() and len(got) == 0 and ctx.homography().matrix is None
        assert int(model["hypothesis"]) == NONE and (model["sample"] == NONE).all() and int(model["matches"]) == 4
        assert_fit(pkg, ctx, M, 64, seed)  # the same list and seed with more hypotheses


def test_collinear_sample_points(pkg):
    with small_context(pkg) as ctx:
        hyp, _, _ = assert_fit(pkg, ctx, collinear_list(64), 256, 0)
    assert 0 < (~hyp["h"].any(axis=1)).sum() < 256


def test_duplicated_records(pkg):
    """SIFT's several orientations at one position: the same coordinates several times.  A sample that
    draws two copies has distinct indices and equal points."""
    M = np.repeat(planted(40), 3)
    M["query"] = np.arange(len(M))
    with small_context(pkg) as ctx:
        hyp, model, got = assert_fit(pkg, ctx, M, 256, 1)
    assert matrix(model) is not None and len(got) == 3 * 28


def test_nan_inf_and_random_bytes(pkg):
    rng = np.random.default_rng(8)
    P = planted(200).copy()
    P["qx"][::7], P["qy"][2::17], P["ty"][3::11], P["tx"][5::13] = np.nan, -np.inf, np.inf, -np.inf
    R = np.frombuffer(rng.bytes(32 * 700), MATCH_DT).copy()
    R["query"] = np.arange(len(R))  # the download's order
    with small_context(pkg) as ctx:
        _, model, got = assert_fit(pkg, ctx, P, 256, 1, what="nan / inf")
        assert matrix(model) is not None and np.isfinite(got["qx"]).all() and 40 < len(got) < 140
        assert_fit(pkg, ctx, R, MAX_H, 2, what="random bytes")
        both = np.concatenate([R[:300], planted(500)])
        both["query"] = np.arange(len(both))  # unique again: the download sorts by `query` alone
        _, model, got = assert_fit(pkg, ctx, both, MAX_H, 3, what="random bytes and a planted model")
        assert matrix(model) is not None and len(got) >= 350


def test_threshold_zero_and_min_inliers(pkg):
    M = planted(100)
    with small_context(pkg) as ctx:
        assert_fit(pkg, ctx, M, 128, 0, threshold=0.0)
        assert_fit(pkg, ctx, collinear_list(64), 256, 0, threshold=0.0)  # integer coordinates: e == 0 does occur
        assert len(ctx.inliers()) >= 4
        _, model, got = assert_fit(pkg, ctx, M, 128, 0)
        count = int(model["inliers"])
        assert count == len(got) == 70
        assert_fit(pkg, ctx, M, 128, 0, min_inliers=count)
        assert ctx.homography().tobytes() == model.tobytes()
        _, none, empty = assert_fit(pkg, ctx, M, 128, 0, min_inliers=count + 1)
        assert matrix(none) is None and len(empty) == 0 and int(none["matches"]) == 100 and ctx.inlier_count() == 0
        for low in (0, 1, 3):
            assert_fit(pkg, ctx, M, 128, 0, min_inliers=low)
            assert ctx.homography().tobytes() == model.tobytes()


# ---------------------------------------------------------------------------------------------
# 3. the pipeline on one stream: build, detect, refine, orient, describe, match, fit
# ---------------------------------------------------------------------------------------------
def raw_matches(pkg, ctx):
    """The match list in DEVICE order: the order the fit read (test plumbing, raw_described's method)."""
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    ctx.sync()
    out = np.zeros(ctx.match_count(), pkg.MATCH_DTYPE)
    if out.size:
        assert hip.hipMemcpy(out.ctypes.data, ctx.device_matches()[0], out.nbytes, 2) == 0  # hipMemcpyDeviceToHost (synchronous)
    return out


def assert_fit_of_the_match_list(pkg, ctx, H, seed, threshold=3.0):
    hyp, model, got = results(ctx)
    M = raw_matches(pkg, ctx)
    assert len(M) >= 4  # the test cannot pass empty
    want_hyp, want_model, want = np_ransac(M, H, seed, threshold)
    assert hyp.tobytes() == want_hyp.tobytes() and model.tobytes() == want_model.tobytes() and got.tobytes() == want.tobytes()
    return M, want_model, want


def test_pipeline_on_one_stream(pkg):
    H, W, S, O = ODD
    with pkg.PyramidContext(H, W, S=S, batch=2) as ctx:
        ctx.upload_pyramid(smooth_pyramid(ODD), 0)
        ctx.upload_pyramid(variant_pyramid(), 1)
        chain(ctx)
        ctx.match_descriptors(query_image=0, train_image=1, ratio=0.8)
        ctx.fit_homography(512, 3)  # the same stream, no synchronisation anywhere above
        M, model, got = assert_fit_of_the_match_list(pkg, ctx, 512, 3)
        print(f"{len(M)} matches: model {matrix(model)}, {len(got)} inliers")
        ctx.fit_homography(64, 4, 1.0)  # again on the same list, other parameters
        assert_fit_of_the_match_list(pkg, ctx, 64, 4, 1.0)
        # image 0 against itself: every match is an inlier of the identity, which every sound sample finds
        ctx.match_descriptors(query_image=0, train_image=0, ratio=0.0)
        ctx.fit_homography(256, 5)
        M, model, got = assert_fit_of_the_match_list(pkg, ctx, 256, 5)
        assert len(got) == len(M) == ctx.described_count(0)
        own = planted(300)  # a caller's list, then back to the match list
        assert_fit(pkg, ctx, own, 128, 1)
        ctx.set_ransac_input(None)
        ctx.fit_homography(256, 5)
        assert ctx.inliers().tobytes() == got.tobytes() and ctx.homography().tobytes() == model.tobytes()


def test_two_contexts_of_different_geometry(pkg, oracle):
    with pkg.PyramidContext(64, 64, S=2) as a, pkg.PyramidContext(48, 80, S=3) as b:
        for ctx, seed in ((a, 12345), (b, 777)):
            ctx.set_input(oracle.lcg_image(ctx.H, ctx.W, seed))
            ctx.build_gaussian()
            ctx.detect_extrema()
            ctx.refine_keypoints(0.5, 10.0)
            ctx.orient_keypoints()
            ctx.describe_keypoints()
        b.sync()
        a.match_descriptors(b, ratio=0.0)
        a.fit_homography(300, 9, 5.0)
        assert_fit_of_the_match_list(pkg, a, 300, 9, 5.0)
        a.match_descriptors(ratio=0.0)  # a against itself: a new match object, so a new fit object
        a.fit_homography(100, 1)
        M, model, got = assert_fit_of_the_match_list(pkg, a, 100, 1)
        assert len(got) == len(M) and matrix(model) is not None
    # both contexts are closed: the fit objects went before the match objects they read


# ---------------------------------------------------------------------------------------------
# 4. state: the fit only reads; a second fit leaves nothing of the first
# ---------------------------------------------------------------------------------------------
def test_the_context_is_left_as_it_was(pkg, oracle):
    n, S = 64, 2
    with pkg.PyramidContext(n, n, S=S) as ctx:
        ctx.set_input(oracle.lcg_image(n, n, 12345))
        ctx.build()
        ctx.build()
        assert ctx.tuning()["zeros_clean"] == 1
        ctx.detect_extrema()
        ctx.refine_keypoints(0.5, 10.0)
        ctx.orient_keypoints()
        ctx.describe_keypoints()
        ctx.match_descriptors(ratio=0.0)
        state = lambda: (ctx.checksum(0), ctx.keypoints(0).tobytes(), ctx.refined_keypoints(0).tobytes(),  # noqa: E731
                         ctx.oriented_keypoints(0).tobytes(), ctx.described_keypoints(0).tobytes(), ctx.matches().tobytes(),
                         raw_matches(pkg, ctx).tobytes(), ctx.pyramid(0).tobytes())
        before = state()
        ctx.fit_homography(256, 2)
        M, model, got = assert_fit_of_the_match_list(pkg, ctx, 256, 2)
        assert ctx.tuning()["zeros_clean"] == 1  # the next build is still the steady-state one
        assert state() == before and len(before[5]) > 0 and len(got) == len(M)
        ctx.build()
        assert ctx.tuning()["zeros_clean"] == 1 and ctx.checksum(0) == before[0]
        ctx.fit_homography(256, 2)
        assert ctx.homography().tobytes() == model.tobytes() and ctx.inliers().tobytes() == got.tobytes()


def test_a_second_fit_leaves_nothing_of_the_first(pkg):
    big, small = planted(900), planted(70, 1)
    with small_context(pkg) as ctx:
        assert ctx.inlier_count() == 0 and len(ctx.inliers()) == 0 and len(ctx.hypotheses()) == 0  # before any fit
        assert ctx.homography().matrix is None and int(ctx.homography()["matches"]) == 0
        _, _, got = assert_fit(pkg, ctx, big, MAX_H, 0)
        assert len(got) == 630
        _, model, got = assert_fit(pkg, ctx, small, 10, 1)  # fewer hypotheses, fewer inliers
        assert len(ctx.hypotheses()) == 10 and len(got) == 49 == ctx.inlier_count()
        assert_fit(pkg, ctx, big, MAX_H, 0)
        _, none, empty = assert_fit(pkg, ctx, small, 3, 1, min_inliers=1000)  # and none at all
        assert len(ctx.hypotheses()) == 3 and ctx.inlier_count() == 0 and len(empty) == 0 and matrix(none) is None
        recs, count, model_at = ctx.device_inliers()
        assert recs and count and model_at


# ---------------------------------------------------------------------------------------------
# 5. refusals, short downloads, the empty list
# ---------------------------------------------------------------------------------------------
def test_refusals_leave_the_previous_result(pkg):
    M = planted(200)
    with small_context(pkg, 250, 300) as ctx:
        assert_fit(pkg, ctx, M, 300, 0)
        before = tuple(r.tobytes() for r in results(ctx))
        for kw, word in (({"hypotheses": 0}, "hypotheses"), ({"hypotheses": 301}, "hypotheses"), ({"threshold": -1.0}, "threshold"),
                         ({"threshold": float("nan")}, "threshold"), ({"threshold": float("inf")}, "threshold"),
                         ({"threshold": -1e-30}, "threshold")):
            with pytest.raises(pkg.GdpError) as e:
                ctx.fit_homography(**{"hypotheses": 64, **kw})
            assert e.value.status == 1 and word in str(e.value)
            assert tuple(r.tobytes() for r in results(ctx)) == before
        with pytest.raises(pkg.GdpError) as e:
            ctx.set_ransac_input(planted(251))
        assert e.value.status == 1 and "capacity" in str(e.value)
        assert tuple(r.tobytes() for r in results(ctx)) == before
        ctx.fit_homography(300, 0)  # the list still stands
        assert tuple(r.tobytes() for r in results(ctx)) == before
        assert_fit(pkg, ctx, planted(250), 300, 0)  # exactly the capacity is fine
        assert_fit(pkg, ctx, M, 64, 0, threshold=-0.0)  # -0 is >= 0


def test_short_downloads_and_an_empty_list_then_none(pkg):
    L = pkg.lib()
    M = planted(100)
    with small_context(pkg) as ctx:
        ctx.match_descriptors(ratio=0.0)  # nothing was described: the match list is empty
        ctx.fit_homography(16, 0)
        hyp, model, got = results(ctx)
        assert len(got) == 0 and model.matrix is None and int(model["matches"]) == 0 and not hyp["matches"].any() and len(hyp) == 16
        _, _, full = assert_fit(pkg, ctx, M, 65, 0)
        assert len(full) == 70
        assert_short_downloads(lambda *a: L.gdp_download_inliers(ctx._ransac, *a), full)
        hyp = ctx.hypotheses()
        for capacity in (64, 0):
            part = np.zeros(65, pkg.HOMOGRAPHY_DTYPE)
            stored = ctypes.c_size_t(99)
            host = ctypes.c_void_p(part.ctypes.data) if capacity else None
            assert L.gdp_download_hypotheses(ctx._ransac, host, capacity, ctypes.byref(stored)) == 0
            assert stored.value == capacity and part[:capacity].tobytes() == hyp[:capacity].tobytes()
            assert not part[capacity:].tobytes().strip(b"\0")
        assert L.gdp_download_inliers(ctx._ransac, None, 0, None, None) == 0 and L.gdp_download_hypotheses(ctx._ransac, None, 0, None) == 0
        assert L.gdp_download_inliers(ctx._ransac, None, 1, None, None) == 1 and L.gdp_download_hypotheses(ctx._ransac, None, 1, None) == 1
        assert_fit(pkg, ctx, M[:0], 16, 0)  # an empty list is a list
        assert ctx.inlier_count() == 0
        ctx.set_ransac_input(None)  # the (empty) match list again
        ctx.fit_homography(16, 0)
        assert int(ctx.homography()["matches"]) == 0 and len(ctx.inliers()) == 0


# ---------------------------------------------------------------------------------------------
# 6. the C++ example, executed
# ---------------------------------------------------------------------------------------------
def test_cpp_example_gives_the_python_paths_model(pkg, oracle):
    """Two 64 x 64 LCG images, the second moved 16 columns to the right.  The example fits the matches
    sorted by their coordinates, which do not depend on the described lists' device order, so the
    model record's bits and the count must be those of the Python path on the same sorted list."""
    exe = os.path.join(REPO, "examples", "ransac_hip")
    if not os.path.exists(exe):
        subprocess.run(["make", "-s", "-C", os.path.join(REPO, "examples"), "ransac_hip"], check=True)
    n, S, seed, shift = 64, 2, 12345, 16
    out = subprocess.run([exe, str(n), str(S), f"lcg:{seed}", str(shift), "0.5", "10", "0.8", "256", "7", "3.0"], check=True,
                         timeout=120, capture_output=True, text=True).stdout
    print(out)
    head = re.match(r"(\d+) inliers of (\d+) matches\nhypothesis (\d+) inliers (\d+) matches (\d+) sample (\d+) (\d+) (\d+) (\d+)\n", out)
    assert head, out
    bits = [int(word, 16) for row in re.findall(r"^h (\w{8}) (\w{8}) (\w{8})", out, re.M) for word in row]
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
        _, model, got = assert_fit(pkg, a, M, 256, 7)
    assert len(M) >= 4
    want = [len(got), len(M), int(model["hypothesis"]), int(model["inliers"]), int(model["matches"])] + [int(s) for s in model["sample"]]
    assert [int(x) for x in head.groups()] == want
    assert bits == [int(w) for w in model["h"].view(np.uint32)]
    assert HOMOGRAPHY_DT.itemsize == 64
