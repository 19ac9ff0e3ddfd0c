"""The three kernels that compact 32-byte match records per wave (k_match_select, k_ransac_inliers,
k_guided_select: one ballot, one atomic, two 16-byte stores) and the list reference they resolve, at
the wave and block edges of their 256-thread blocks, through the public Python surface on a 32 x 32
context.  Every length runs with every record kept and with a cap or a planted fraction that keeps
about a third, spread over the lanes; every comparison is equality of the downloaded records' bytes
and of `found` with the oracles (match_oracle.np_match, ransac_oracle.np_ransac,
guided_oracle.np_guided).

Not repeated here: gdp_match_descriptors with every record kept (ratio 0, no cap, no mutual test) at
query lengths 0, 1, 63, 64, 65 is test_gpu_match.test_callers_lists_small_lengths, at 255, 256 and 257
test_gpu_match.test_callers_lists_at_the_chunk_seams."""
import functools

import numpy as np
import pytest

from guided_oracle import np_guided
from match_oracle import NONE, distances, np_match
from ransac_oracle import np_ransac, planted_list
from test_gpu_guided import placed
from test_gpu_match import random_records, raw_described
from test_gpu_ransac import raw_matches

pytestmark = pytest.mark.gpu

F = np.float32
IDENTITY = np.eye(3, dtype=F)
SIDE, S = 32, 2
LENGTHS = (0, 1, 63, 64, 65, 255, 256, 257)  # the wave (64) and block (256) edges of the select kernels
CAPACITY, MAX_H = 260, 520
NT = 33  # the other list of the two matching stages: one partial MFMA tile past a whole one


def context(pkg, match=(CAPACITY, CAPACITY), ransac=(CAPACITY, MAX_H), batch=1):
    ctx = pkg.PyramidContext(SIDE, SIDE, S=S, octaves=1, batch=batch)
    ctx.set_match_capacity(*match)
    ctx.set_ransac_capacity(*ransac)
    return ctx


def about_a_third(n, kept):
    """A case that keeps nothing or everything cannot pass silently (one record cannot be a third)."""
    assert n < 2 or n / 4 <= kept <= n / 2, (n, kept)


def cap_for_a_third(distance):
    """The cap below which n // 3 of the distances lie (distinct distances), from the oracle's records."""
    return int(np.sort(distance)[len(distance) // 3]) - 1 if len(distance) else 0


def assert_records(pkg, got, want, what):
    assert got.dtype == pkg.MATCH_DTYPE
    assert got.found == len(want) and got.tobytes() == want.tobytes(), (what, got.found, len(got), len(want))


# ---------------------------------------------------------------------------------------------
# 1. the caller's lists
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def match_lists(n):
    Q, T = random_records(n, 700 + n), random_records(NT, 800 + n)
    D = distances(Q, T)
    return Q, T, D, np_match(Q, T, 0.0, NONE, False, D=D)


@pytest.mark.parametrize("n", LENGTHS)
def test_match_select_keeps_a_third(pkg, n):
    Q, T, D, full = match_lists(n)
    cap = cap_for_a_third(full["distance"])
    want = np_match(Q, T, 0.0, cap, False, D=D)
    assert len(full) == n
    about_a_third(n, len(want))
    with context(pkg) as ctx:
        ctx.set_match_input(0, Q)
        ctx.set_match_input(1, T)
        ctx.match_descriptors(ratio=0.0, max_distance=cap)
        assert_records(pkg, ctx.matches(), want, n)
        assert ctx.match_count() == len(want)


@functools.lru_cache(maxsize=None)
def guided_lists(n):
    rng = np.random.default_rng(900 + n)
    Q = placed(rng.uniform(0, SIDE, (n, 2)), 1000 + n)
    T = placed(rng.uniform(0, SIDE, (NT, 2)), 1100 + n)
    D = distances(Q, T)
    return Q, T, D, np_guided(Q, T, IDENTITY, 1e9, 0.0, NONE, False, D=D)


@pytest.mark.parametrize("n", LENGTHS)
def test_guided_select_keeps_all_and_a_third(pkg, n):
    Q, T, D, full = guided_lists(n)
    cap = cap_for_a_third(full["distance"])
    third = np_guided(Q, T, IDENTITY, 1e9, 0.0, cap, False, D=D)
    assert len(full) == n  # a window of 1e9 pixels holds every train record
    about_a_third(n, len(third))
    with context(pkg) as ctx:
        ctx.set_match_input(0, Q)
        ctx.set_match_input(1, T)
        ctx.set_guided_model(IDENTITY)
        for max_distance, want in ((None, full), (cap, third)):
            ctx.guided_match(1e9, ratio=0.0, max_distance=max_distance, unique=False)
            assert_records(pkg, ctx.guided_matches(), want, (n, max_distance))
            assert ctx.guided_count() == len(want)


@functools.lru_cache(maxsize=None)
def ransac_lists(n):
    """(a list every record of which fits the planted model, a list of which 36 in 100 do)."""
    return planted_list(n, n, 1200 + n, noise=0.0)[0], planted_list(n, (9 * n + 24) // 25, 1300 + n)[0]


@pytest.mark.parametrize("n", LENGTHS)
def test_ransac_inliers_keeps_all_and_a_third(pkg, n):
    every, some = ransac_lists(n)
    with context(pkg) as ctx:
        for M, whole in ((every, True), (some, False)):
            want_hyp, want_model, want = np_ransac(M, MAX_H, 1, 3.0)
            if n >= 4 and whole:
                assert len(want) == n
            elif n >= 4:
                about_a_third(n, len(want))
            else:
                assert len(want) == 0  # no sample of four: no model
            ctx.set_ransac_input(M)
            ctx.fit_homography(MAX_H, 1, 3.0)
            assert_records(pkg, ctx.inliers(), want, (n, whole))
            assert ctx.inlier_count() == len(want)
            assert ctx.homography().tobytes() == want_model.tobytes() and ctx.hypotheses().tobytes() == want_hyp.tobytes()


# ---------------------------------------------------------------------------------------------
# 2. the producer's lists, longer than the consumer's capacity: the first `capacity` records are read
# ---------------------------------------------------------------------------------------------
def test_a_producers_counter_above_the_consumers_capacity_is_clamped(pkg):
    """Image 0 gets 40 described records and image 1 gets 36; the match object holds 24 and 20, the
    fit object 16.  The describe input is the caller's (every interior sample of a random pyramid has
    a descriptor), so no count depends on the detection."""
    rng = np.random.default_rng(5)
    levels = (S + 3) * SIDE * SIDE
    described = (40, 36)
    with context(pkg, match=(24, 20), ransac=(16, 64), batch=2) as ctx:
        for b, n in enumerate(described):
            ctx.upload_pyramid(rng.standard_normal(levels).astype(F), b)
            recs = np.zeros(n, pkg.ORIENTED_DTYPE)
            recs["scale"], recs["kind"] = rng.integers(1, S + 1, n), 1
            recs["row"], recs["col"] = rng.integers(1, SIDE - 1, n), rng.integers(1, SIDE - 1, n)
            recs["drow"], recs["dcol"] = rng.uniform(-0.5, 0.5, n), rng.uniform(-0.5, 0.5, n)
            recs["angle"] = rng.uniform(0, 359, n)
            ctx.set_describe_input(recs, b)
        ctx.describe_keypoints()
        assert (ctx.described_count(0), ctx.described_count(1)) == described
        Q, T = raw_described(pkg, ctx, 0)[:24], raw_described(pkg, ctx, 1)[:20]

        ctx.match_descriptors(query_image=0, train_image=1, ratio=0.0)
        want = np_match(Q, T)
        assert len(want) == 24
        assert_records(pkg, ctx.matches(), want, "match")

        ctx.fit_homography(64, 3, 1e4)  # the match counter says 24, the fit object holds 16
        M = raw_matches(pkg, ctx)
        assert len(M) == 24
        want_hyp, want_model, want = np_ransac(M[:16], 64, 3, 1e4)
        assert int(want_model["matches"]) == 16
        assert ctx.hypotheses().tobytes() == want_hyp.tobytes() and ctx.homography().tobytes() == want_model.tobytes()
        assert_records(pkg, ctx.inliers(), want, "ransac")

        ctx.set_guided_model(IDENTITY)
        ctx.guided_match(1e9, unique=False, query_image=0, train_image=1)
        want = np_guided(Q, T, IDENTITY, 1e9, unique=False)
        assert len(want) == 24
        assert_records(pkg, ctx.guided_matches(), want, "guided")
