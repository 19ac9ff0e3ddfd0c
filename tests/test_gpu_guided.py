"""On-device guided matching (gdp_match_guided) against the literal numpy oracle of
tests/guided_oracle.py, which tests every pair and knows no grid.  Distances are exact integers, the
window is four float32 comparisons and ties have a total order, so the result is an exact set: every
comparison is equality of the downloaded records' bytes with the oracle's.  The synthetic cases run on
test_gpu_match.small_context (40 x 56) with the caller's lists (set_match_input) and the caller's
model (set_guided_model): a record's coordinates are its (dcol, drow) with row = col = octave = 0, so a
point is placed exactly."""
import functools
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

from guided_oracle import candidates, np_guided, windows
from match_oracle import NONE, distances
from ransac_oracle import NONE as NO_MODEL
from test_gpu_match import chain, random_records, raw_described, small_context
from test_gpu_ransac import raw_matches
from test_gpu_warp import QH, QW, ROTATION, TH, TW, run_chain, scene, shift

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
IDENTITY = np.eye(3, dtype=F)
W, H = 56, 40  # small_context's frame
LENGTHS = (0, 1, 2, 7, 8, 9, 63, 64, 65, 257)  # the lane-group (8), wave (64) and block (32 queries, 256 threads) seams


def placed(xy, seed, spread=None):
    """One record per (x, y), placed exactly; random descriptors, or (spread) noisy copies of one
    descriptor so that the ratio test has something to decide."""
    xy = np.asarray(xy, F).reshape(-1, 2)
    R = random_records(len(xy), seed)
    R["octave"], R["row"], R["col"] = 0, 0, 0
    R["dcol"], R["drow"] = xy[:, 0], xy[:, 1]
    if spread is not None and len(xy):
        rng = np.random.default_rng(seed)
        base = rng.integers(0, 256, 128)
        R["desc"] = np.clip(base + rng.integers(-spread, spread + 1, (len(xy), 128)), 0, 255)
    return R


@functools.lru_cache(maxsize=None)
def random_list(n, seed):
    rng = np.random.default_rng(seed)
    R = placed(np.stack([rng.uniform(0, W, n), rng.uniform(0, H, n)], 1), seed, spread=20)
    R.setflags(write=False)
    return R


def load(ctx, Q, T, h):
    ctx.set_match_input(0, Q)
    ctx.set_match_input(1, T)
    ctx.set_guided_model(h)


def run(ctx, radius, **kw):
    ctx.guided_match(radius, **kw)
    got = ctx.guided_matches()
    assert got.found == ctx.guided_count() == len(got)
    return got


def assert_guided(pkg, ctx, Q, T, h, radius, ratio=0.0, max_distance=None, unique=True, D=None, what=None, stats=None):
    got = run(ctx, radius, ratio=ratio, max_distance=max_distance, unique=unique)
    want = np_guided(Q, T, h, radius, ratio, NONE if max_distance is None else max_distance, unique, D=D, stats=stats)
    assert got.dtype == pkg.MATCH_DTYPE
    assert got.tobytes() == want.tobytes(), (what, radius, ratio, max_distance, unique, len(got), len(want))
    return want


def spans(Q, h, radius, side, gx, gy):
    """Cells per axis that the windows touch, as the rule's cell index gives them (the oracle knows no cells)."""
    x0, x1, y0, y1, has = windows(Q, h, radius)
    cell = lambda v, g: np.clip(np.floor(v * F(1 / side)), 0, g - 1)  # noqa: E731
    return {int(n) for n in (cell(x1, gx) - cell(x0, gx) + 1)[has]} | {int(n) for n in (cell(y1, gy) - cell(y0, gy) + 1)[has]}


# ---------------------------------------------------------------------------------------------
# 1. lengths at the lane-group, wave and block seams, nq = 0 and nt = 0 included
# ---------------------------------------------------------------------------------------------
def test_lengths_at_the_group_wave_and_block_seams(pkg):
    kept = np.zeros(3, np.int64)
    with small_context(pkg) as ctx:
        for nq, nt in itertools.product(LENGTHS, LENGTHS):
            Q, T = random_list(nq, 100 + nq), random_list(nt, 200 + nt)
            load(ctx, Q, T, IDENTITY)
            D = distances(Q, T)
            stats = {}
            kept[0] += len(assert_guided(pkg, ctx, Q, T, IDENTITY, 6.0, unique=False, D=D, what=(nq, nt)))
            kept[1] += len(assert_guided(pkg, ctx, Q, T, IDENTITY, 6.0, 0.9, unique=False, D=D, what=(nq, nt)))
            kept[2] += len(assert_guided(pkg, ctx, Q, T, IDENTITY, 6.0, unique=True, D=D, what=(nq, nt), stats=stats))
    print("kept over the 100 pairs (plain, ratio 0.9, unique):", kept)
    assert kept[0] > kept[1] > 0 and kept[0] > kept[2] > 0  # both filters keep some and drop some


# ---------------------------------------------------------------------------------------------
# 2. cell seams, placed from guided_layout()
# ---------------------------------------------------------------------------------------------
def seam_points(side):
    """Points exactly on multiples of the cell side and one ulp to either side of them, on both axes:
    the first and the last seam of the frame (the last lies past its last cell) and two between."""
    def axis(extent):
        ks = sorted(set(np.linspace(0, int(extent // side) + 1, 4).astype(int)))
        return [v for k in ks for v in (np.nextafter(F(k * side), F(-1e9)), F(k * side), np.nextafter(F(k * side), F(1e9)))]

    return np.array(list(itertools.product(axis(W), axis(H))), F)


@pytest.mark.parametrize("radius", [0.0, 0.25, 0.75, 1.0, 2.0, 3.0, 4.0, 6.5, 16.0])
def test_trains_on_the_cell_seams_and_windows_ending_on_a_train(pkg, radius):
    with small_context(pkg) as ctx:
        load(ctx, placed([(1, 1)], 1), placed([(1, 1)], 2), IDENTITY)
        run(ctx, radius)
        side, gx, gy, most, lanes = ctx.guided_layout()
        assert lanes == 8 and most == 1 << 18 and side == max(1.0, 2.0 ** np.ceil(np.log2(max(radius / 2, 1e-9))))
        assert (gx, gy) == (int(np.ceil(W / side)), int(np.ceil(H / side)))
        T = placed(seam_points(side), 3)
        # queries whose window edges are exactly train coordinates (inclusive on both sides), one ulp short of them, and on them
        t = np.asarray([T["dcol"], T["drow"]], F).T[:: max(1, len(T) // 40)]
        r = F(radius)
        Q = placed(np.concatenate([t + r, t - r, np.nextafter(t + r, F(1e9)), np.nextafter(t - r, F(-1e9)), t]), 4)
        load(ctx, Q, T, IDENTITY)
        stats = {}
        want = assert_guided(pkg, ctx, Q, T, IDENTITY, radius, unique=False, what="seams", stats=stats)
        assert_guided(pkg, ctx, Q, T, IDENTITY, radius, unique=True, what="seams")
        C = candidates(Q, T, IDENTITY, radius)
        x0, x1, _, _, _ = windows(Q, IDENTITY, radius)
        edge_hits = int(((x0[:, None] == T["dcol"][None, :]) & C).sum() + ((x1[:, None] == T["dcol"][None, :]) & C).sum())
        print(f"radius {radius}: side {side}, grid {gx} x {gy}, {len(T)} trains, {len(Q)} queries, {len(want)} records, "
              f"{edge_hits} candidates on a window edge, spans {sorted(spans(Q, IDENTITY, radius, side, gx, gy))}")
        assert len(want) > 0 and edge_hits > 0 and (radius == 0 or stats["multi"] > 0)
        assert ctx.guided_layout()[:3] == (side, gx, gy)


def test_windows_span_one_to_five_cells_per_axis(pkg):
    """The cell side follows the radius, so the spans are read from the layout, not assumed."""
    seen = set()
    with small_context(pkg) as ctx:
        rng = np.random.default_rng(5)
        Q = placed(np.stack([rng.uniform(-3, W + 3, 90), rng.uniform(-3, H + 3, 90)], 1).round(1), 6, spread=10)
        T = placed(np.stack([rng.uniform(-3, W + 3, 400), rng.uniform(-3, H + 3, 400)], 1).round(1), 7, spread=10)
        load(ctx, Q, T, IDENTITY)
        D = distances(Q, T)
        for radius in (0.0, 0.3, 0.75, 1.5, 3.0, 4.0, 8.0):
            assert_guided(pkg, ctx, Q, T, IDENTITY, radius, D=D, what="spans")
            side, gx, gy = ctx.guided_layout()[:3]
            seen |= spans(Q, IDENTITY, radius, side, gx, gy)
    print("cells per axis seen:", sorted(seen))
    assert {1, 2, 3} <= seen and max(seen) >= 4


def test_one_cell_the_most_cells_a_raised_side_and_two_radii_on_one_object(pkg):
    rng = np.random.default_rng(8)
    Q = placed(np.stack([rng.uniform(0, W, 70), rng.uniform(0, H, 70)], 1), 9, spread=10)
    T = placed(np.stack([rng.uniform(0, W, 300), rng.uniform(0, H, 300)], 1), 10, spread=10)
    D = distances(Q, T)
    with small_context(pkg) as ctx:
        load(ctx, Q, T, IDENTITY)
        layouts = []
        # the most cells (side 1: 56 x 40), one cell, the most again: a histogram or a cursor that is not reset would show
        for radius in (0.5, 1e9, 2.0, 200.0, 0.0, 3.0, 3e38, 1.0):
            assert_guided(pkg, ctx, Q, T, IDENTITY, radius, D=D, what="two radii")
            assert_guided(pkg, ctx, Q, T, IDENTITY, radius, 0.8, unique=False, D=D, what="two radii")
            layouts.append(ctx.guided_layout()[:3])
        assert layouts[0] == (1.0, W, H) == layouts[2] == layouts[4] == layouts[7] and layouts[5] == (2.0, W // 2, H // 2)
        assert layouts[1] == (2.0 ** 29, 1, 1) and layouts[3] == (128.0, 1, 1) and layouts[6] == (2.0 ** 64, 1, 1)
        # a bound of 64 cells raises the side until the frame fits: 8 x 5 cells of side 8 at any small radius
        ctx.set_guided_capacity(64)
        load(ctx, Q, T, IDENTITY)
        for radius in (0.0, 3.0, 20.0):
            assert_guided(pkg, ctx, Q, T, IDENTITY, radius, D=D, what="raised")
            assert ctx.guided_layout() == ((8.0, 7, 5, 64, 8) if radius < 20 else (16.0, 4, 3, 64, 8))
        ctx.set_guided_capacity(1)
        load(ctx, Q, T, IDENTITY)
        assert_guided(pkg, ctx, Q, T, IDENTITY, 3.0, D=D, what="one cell by the bound")
        assert ctx.guided_layout() == (64.0, 1, 1, 1, 8)


# ---------------------------------------------------------------------------------------------
# 3. coordinates outside the frame clamp into the edge cells and are no wrong candidates
# ---------------------------------------------------------------------------------------------
def test_coordinates_outside_the_frame(pkg):
    odd = [(-5.0, -7.0), (-0.0, 0.0), (W + 9.0, 3.0), (3.0, H + 11.0), (W + 2.0, H + 2.0), (1e30, 5.0), (5.0, -1e30), (np.inf, 5.0),
           (5.0, -np.inf), (-np.inf, np.inf), (-np.inf, 5.0), (np.nan, 5.0), (5.0, np.nan), (np.nan, np.nan), (W - 0.5, H - 0.5), (W, H)]
    T = np.concatenate([placed(odd, 11), placed(odd, 12), placed([(3.0, 4.0)], 13)])
    T["octave"][-1] = 31 + 32  # octave & 31 = 31: (3 * 2^31, 4 * 2^31)
    Q = np.concatenate([placed(odd, 14), placed([(3.0, 4.0)], 15), placed([(-4.0, -6.0), (W + 8.0, 2.0), (2.0, H + 10.0)], 16)])
    Q["octave"][len(odd)] = 31
    D = distances(Q, T)
    # an infinite query coordinate makes w a NaN (0 * inf); an infinite WINDOW comes from a product that overflows
    models = {"identity": IDENTITY, "overflow": np.array([[1e30, 0, 0], [0, 1, 0], [0, 0, 1]], F),
              "negative overflow": np.array([[-1e30, 0, 0], [0, 1, 0], [0, 0, 1]], F)}
    seen = 0
    with small_context(pkg) as ctx:
        for name, h in models.items():
            load(ctx, Q, T, h)
            for radius in (0.0, 1.5, 12.0, 1e9, 3e38):
                for unique in (False, True):
                    seen += len(assert_guided(pkg, ctx, Q, T, h, radius, unique=unique, D=D, what=("outside", name)))
            C = candidates(Q, T, h, 3e38)
            assert not C[:, np.isnan(T["dcol"]) | np.isnan(T["drow"])].any()
        for name in ("overflow", "negative overflow"):
            inf_hits = candidates(Q, T, models[name], 0.0)[:, np.isinf(T["dcol"]) & (T["drow"] == 5)].sum()
            assert inf_hits > 0, name  # inf <= inf && inf <= inf: an infinite train IS a candidate of an infinite window
    assert seen > 0


# ---------------------------------------------------------------------------------------------
# 4. a crowded cell: 1,025 trains at one position, identical descriptors among them
# ---------------------------------------------------------------------------------------------
def test_a_crowded_cell(pkg):
    rng = np.random.default_rng(17)
    T = placed(np.tile([(20.25, 10.5)], (1025, 1)), 18, spread=3)
    T["desc"][rng.permutation(1025)[:200]] = T["desc"][700]  # 201 identical descriptors: the lowest index wins
    Q = placed(np.tile([(20.0, 10.0)], (9, 1)), 19, spread=3)
    Q["desc"][0] = T["desc"][700]
    Q["desc"][1] = T["desc"][3]
    with small_context(pkg) as ctx:
        load(ctx, Q, T, IDENTITY)
        D = distances(Q, T)
        for radius in (0.5, 3.0, 1e9):
            want = assert_guided(pkg, ctx, Q, T, IDENTITY, radius, unique=False, D=D, what="crowded")
            assert_guided(pkg, ctx, Q, T, IDENTITY, radius, unique=True, D=D, what="crowded")
        first = int(np.flatnonzero((T["desc"] == T["desc"][700]).all(axis=1))[0])
        assert len(want) == 9 and first < 700 and (int(want["train"][0]), int(want["distance"][0]), int(want["second"][0])) == (first, 0, 0)
        assert len(run(ctx, 0.25)) == 0  # nothing within a quarter pixel


# ---------------------------------------------------------------------------------------------
# 5. a single candidate, and the ratio and cap seams
# ---------------------------------------------------------------------------------------------
def test_a_single_candidate_and_the_filter_seams(pkg):
    def ones(k, xy):
        r = placed([xy], k)
        r["desc"] = 0
        r["desc"][0, :k] = 1
        return r

    Q = ones(0, (10.0, 10.0))
    with small_context(pkg) as ctx:
        seen = set()
        for distance, second, ratio in ((16, 25, 0.8), (25, 100, 0.5), (64, 100, 0.8), (9, 25, 0.6), (36, 100, 0.6), (1, 4, 0.5),
                                        (49, 100, 0.7), (16, 25, 0.81), (16, 25, 0.79)):
            T = np.concatenate([ones(second, (11.0, 10.0)), ones(distance, (10.0, 11.0)), ones(0, (30.0, 30.0))])  # the last: outside
            load(ctx, Q, T, IDENTITY)
            want = assert_guided(pkg, ctx, Q, T, IDENTITY, 2.0, ratio, what=(distance, second, ratio))
            seen.add(len(want))
            if len(want):
                assert (int(want["train"][0]), int(want["distance"][0]), int(want["second"][0])) == (1, distance, second)
            assert len(run(ctx, 2.0, max_distance=distance)) == 1  # the cap is inclusive
            assert len(run(ctx, 2.0, max_distance=distance - 1)) == 0
            assert len(run(ctx, 2.0, max_distance=0xFFFFFFFF)) == 1
            # a window that holds train 1 only: second = 0xffffffff, and every ratio passes
            ctx.set_guided_model(shift(0, 1))
            for r in (0.0, 1e-3, 0.5, 1.0):
                one = assert_guided(pkg, ctx, Q, T, shift(0, 1), 0.5, r, what="single")
                assert (int(one["train"][0]), int(one["distance"][0]), int(one["second"][0])) == (1, distance, NONE)
        assert seen == {0, 1}


# ---------------------------------------------------------------------------------------------
# 6. models
# ---------------------------------------------------------------------------------------------
def test_models(pkg):
    rng = np.random.default_rng(20)
    Q = placed(np.stack([rng.uniform(0, W, 120), rng.uniform(0, H, 120)], 1).round(2), 21, spread=10)
    T = placed(np.stack([rng.uniform(-10, W + 20, 500), rng.uniform(-10, H + 20, 500)], 1).round(2), 22, spread=10)
    D = distances(Q, T)
    nan_entry = ROTATION.copy()
    nan_entry[1, 1] = np.nan
    models = {"identity": IDENTITY, "shift": shift(5.5, -3.25), "rotation": ROTATION,
              "w crosses": np.array([[1, 0, 0], [0, 1, 0], [-1, 0, 20]], F),  # w = 20 - x: no window for x >= 20
              "none": np.zeros((3, 3), F), "nan": nan_entry, "w nan": np.array([[1, 0, 0], [0, 1, 0], [0, 0, np.nan]], F),
              "negative": -IDENTITY}
    with small_context(pkg) as ctx:
        for name, h in models.items():
            load(ctx, Q, T, h)
            for radius, unique in ((4.0, False), (4.0, True), (0.75, True)):
                want = assert_guided(pkg, ctx, Q, T, h, radius, unique=unique, D=D, what=name)
                if name in ("none", "nan", "w nan", "negative"):
                    assert len(want) == 0
                elif radius == 4.0:
                    assert len(want) > 0
        _, _, _, _, has = windows(Q, models["w crosses"], 4.0)
        assert 0 < has.sum() < len(Q)
        ctx.set_guided_model(None)  # the fit object's record before any fit is the "none" record
        assert len(run(ctx, 4.0)) == 0


# ---------------------------------------------------------------------------------------------
# 7. descriptor extremes and the byte order of the dot products
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("q,t,distance", [(0, 255, 8323200), (255, 255, 0), (128, 127, 128), (255, 0, 8323200)])
def test_value_extremes(pkg, q, t, distance):
    Q, T = placed([(5, 5), (6, 5), (30, 30)], 23), placed([(5, 6), (6, 6)], 24)
    Q["desc"], T["desc"] = q, t
    with small_context(pkg) as ctx:
        load(ctx, Q, T, IDENTITY)
        want = assert_guided(pkg, ctx, Q, T, IDENTITY, 2.0, unique=False, what="extremes")
    assert len(want) == 2 and (want["distance"] == distance).all() and (want["second"] == distance).all() and (want["train"] == 0).all()


def test_one_hot_byte_order(pkg):
    Q, T = placed(np.tile([(9.0, 9.0)], (128, 1)), 25), placed(np.tile([(9.5, 9.5)], (128, 1)), 26)
    Q["desc"], T["desc"] = 0, 0
    for i in range(128):
        Q["desc"][i, i] = 200
        T["desc"][i, 127 - i] = 180
    with small_context(pkg) as ctx:
        load(ctx, Q, T, IDENTITY)
        want = assert_guided(pkg, ctx, Q, T, IDENTITY, 1.0, unique=False, what="one hot")
    assert list(want["train"]) == [127 - i for i in range(128)]
    assert (want["distance"] == 400).all() and (want["second"] == 200 * 200 + 180 * 180).all()


# ---------------------------------------------------------------------------------------------
# 8. unique
# ---------------------------------------------------------------------------------------------
def test_unique_keeps_one_query_per_train(pkg):
    T = placed([(10, 10), (30, 30), (12, 10)], 27)
    Q = placed([(10, 10), (10.5, 10), (10, 10.5), (30, 30), (9.5, 10)], 28)
    Q["desc"][[0, 1, 4]] = T["desc"][0]
    Q["desc"][0, 0] ^= 4  # queries 0 and 1: distance 16, query 4: 64, query 2: 0
    Q["desc"][1, 0] ^= 4
    Q["desc"][4, 0] ^= 8
    Q["desc"][2] = T["desc"][0]
    with small_context(pkg) as ctx:
        load(ctx, Q, T, IDENTITY)
        both = assert_guided(pkg, ctx, Q, T, IDENTITY, 1.0, unique=False, what="not unique")
        one = assert_guided(pkg, ctx, Q, T, IDENTITY, 1.0, unique=True, what="unique")
        assert both["train"].tolist() == [0, 0, 0, 1, 0] and one["query"].tolist() == [2, 3]
        # a loser is absent: at radius 2 query 1 also sees train 2, and is not matched to it
        assert assert_guided(pkg, ctx, Q, T, IDENTITY, 2.0, unique=True, what="absent")["query"].tolist() == [2, 3]
        sub = Q[[0, 1, 3, 4]]  # equal distances: the lowest query
        load(ctx, sub, T, IDENTITY)
        assert assert_guided(pkg, ctx, sub, T, IDENTITY, 1.0, unique=True, what="tie")["query"].tolist() == [0, 2]
        many = placed(np.tile([(10.0, 10.0)], (300, 1)), 29)  # 300 claimants of one train over several blocks
        many["desc"] = T["desc"][0]
        load(ctx, many, T, IDENTITY)
        assert assert_guided(pkg, ctx, many, T, IDENTITY, 1.0, unique=True, what="many")["query"].tolist() == [0]


# ---------------------------------------------------------------------------------------------
# 9. the pipeline on one stream: build ... match, fit, guided match, with no host read in between
# ---------------------------------------------------------------------------------------------
def test_pipeline_on_one_stream(pkg, oracle):
    qimg, timg = scene(oracle)
    radius, ratio = 3.0, 0.8
    with pkg.PyramidContext(QH, QW, S=2, octaves=2) as q, pkg.PyramidContext(TH, TW, S=2, octaves=2) as t:
        run_chain(q, t, qimg, timg)
        q.match_descriptors(t, ratio=0.0)
        q.fit_homography(512, 3, 2.0)
        q.guided_match(radius, ratio=ratio, unique=True)  # the same stream, no synchronisation and no host read above
        got = q.guided_matches()
        q.guided_match(radius, ratio=ratio, unique=True)  # the counter and the grid are zeroed again
        again = q.guided_matches()
        Q, T = raw_described(pkg, q, 0), raw_described(pkg, t, 0)
        model = q.homography()
        assert model.matrix is not None and int(model["hypothesis"]) != NO_MODEL
        stats = {}
        want = np_guided(Q, T, model["h"], radius, ratio, stats=stats)
        loose = np_guided(Q, T, model["h"], radius, 0.0, unique=False)
        print(f"{len(Q)} x {len(T)} described records, {len(raw_matches(pkg, q))} dense matches, {int(model['inliers'])} inliers: "
              f"{len(loose)} queries with a candidate, {len(want)} guided records, {stats}")
        # the test is not vacuous: conditions on the inputs, taken from the oracle's result
        assert len(want) >= 16 and stats["multi"] >= 1 and stats["ratio_dropped"] >= 1 and stats["unique_dropped"] >= 1
        assert got.tobytes() == want.tobytes() == again.tobytes()
        assert len(set(got["train"])) == len(got)  # one-to-one
        # what a second fit wants: the guided list through set_ransac_input
        q.set_ransac_input(got)
        q.fit_homography(256, 5, 2.0)
        assert q.homography().matrix is not None
        # the "none" record: nothing is output
        q.set_ransac_input(None)
        q.fit_homography(64, 3, 2.0, min_inliers=len(Q) + 1)
        assert int(q.homography()["hypothesis"]) == NO_MODEL and len(run(q, radius)) == 0


# ---------------------------------------------------------------------------------------------
# 10. state: guided matching only reads
# ---------------------------------------------------------------------------------------------
def test_everything_upstream_is_left_as_it_was(pkg, oracle):
    qimg, timg = scene(oracle)
    with pkg.PyramidContext(QH, QW, S=2, octaves=2) as q, pkg.PyramidContext(TH, TW, S=2, octaves=2) as t:
        for ctx, img in ((q, qimg), (t, timg)):
            ctx.set_input(img)
            ctx.build()
            ctx.build()
            assert ctx.tuning()["zeros_clean"] == 1
            chain(ctx)
        t.sync()
        q.match_descriptors(t, ratio=0.0)
        q.fit_homography(128, 2, 2.0)

        def state():
            per_ctx = tuple((c.checksum(0), c.pyramid(0).tobytes(), c.keypoints(0).tobytes(), c.refined_keypoints(0).tobytes(),
                             c.oriented_keypoints(0).tobytes(), c.described_keypoints(0).tobytes(), c.tuning()["zeros_clean"])
                            for c in (q, t))
            return per_ctx + (q.matches().tobytes(), raw_matches(pkg, q).tobytes(), q.hypotheses().tobytes(), q.homography().tobytes(),
                              q.inliers().tobytes())

        before = state()
        assert before[0][6] == before[1][6] == 1 and len(before[3]) > 0
        Q, T = raw_described(pkg, q, 0), raw_described(pkg, t, 0)
        for unique in (False, True):
            got = run(q, 3.0, ratio=0.8, unique=unique)
            assert got.tobytes() == np_guided(Q, T, q.homography()["h"], 3.0, 0.8, unique=unique).tobytes() and len(got) > 0
            assert state() == before
        q.set_guided_model(ROTATION)
        assert run(q, 5.0).tobytes() == np_guided(Q, T, ROTATION, 5.0).tobytes()
        assert state() == before
        for ctx in (q, t):  # the next build is still the steady-state one
            ctx.build()
            assert ctx.tuning()["zeros_clean"] == 1
        assert (q.checksum(0), t.checksum(0)) == (before[0][0], before[1][0])


# ---------------------------------------------------------------------------------------------
# 11. refusals, a batch of three, the C++ example
# ---------------------------------------------------------------------------------------------
def test_refusals_leave_the_previous_result(pkg):
    Q, T = random_list(65, 30), random_list(257, 31)
    with small_context(pkg) as ctx:
        load(ctx, Q, T, IDENTITY)
        want = assert_guided(pkg, ctx, Q, T, IDENTITY, 6.0, what="before")
        layout = ctx.guided_layout()
        assert len(want) > 0
        for radius in (float("nan"), -1.0, -1e-30, float("inf"), float("-inf")):
            with pytest.raises(pkg.GdpError) as e:
                ctx.guided_match(radius)
            assert e.value.status == 1 and "radius" in str(e.value)
        for ratio in (float("nan"), -0.5, 1.5, float("inf")):
            with pytest.raises(pkg.GdpError) as e:
                ctx.guided_match(6.0, ratio=ratio)
            assert e.value.status == 1 and "ratio" in str(e.value)
        for kw in ({"query_image": 1}, {"train_image": 1}, {"query_image": -1}, {"train_image": -1}):
            with pytest.raises(pkg.GdpError) as e:
                ctx.guided_match(6.0, **kw)
            assert e.value.status == 1 and "image" in str(e.value)
        with pytest.raises(ValueError):
            ctx.set_guided_model(np.zeros(8, F))
        got = ctx.guided_matches()
        assert got.tobytes() == want.tobytes() and ctx.guided_layout() == layout  # the previous result, still downloadable
        assert pkg.lib().gdp_download_guided(ctx._handles["guided"], None, 4, None, None) == 1
        assert_guided(pkg, ctx, Q, T, IDENTITY, 6.0, 1.0, what="the closed end of (0, 1]")
        assert_guided(pkg, ctx, Q, T, IDENTITY, -0.0, what="minus zero is zero")
    with pytest.raises(pkg.GdpError) as e:
        with small_context(pkg) as ctx:
            ctx.set_guided_capacity((1 << 24) + 1)
            ctx.guided_match(1.0)
    assert e.value.status == 1 and "cells" in str(e.value)


def test_batch_three_picks_its_images(pkg, oracle):
    H3, W3, S = 64, 64, 2
    with pkg.PyramidContext(H3, W3, S=S, octaves=2, batch=3) as ctx:
        for b in range(3):
            ctx.set_input(oracle.lcg_image(H3, W3, 100 + b), b)
        ctx.build_gaussian()
        ctx.detect_extrema()
        ctx.refine_keypoints(0.5, 10.0)
        ctx.orient_keypoints()
        ctx.describe_keypoints()
        lists = [raw_described(pkg, ctx, b) for b in range(3)]
        assert all(len(r) > 8 for r in lists)
        ctx.match_descriptors(ratio=0.0)
        ctx.set_guided_model(IDENTITY)
        for qi, ti in ((2, 1), (0, 2), (1, 1)):
            got = run(ctx, 12.0, query_image=qi, train_image=ti)
            want = np_guided(lists[qi], lists[ti], IDENTITY, 12.0)
            assert got.tobytes() == want.tobytes() and len(want) > 0, (qi, ti)


def test_cpp_example_prints_the_python_paths_records(pkg, oracle):
    """Two 64 x 64 LCG images, the second moved 16 columns to the right, matched under the caller's
    translation.  The described lists' device order, which the indices name, may differ between the
    two processes: the counts must be equal, and each of the example's lines, without its two
    indices, must be a record of the Python path."""
    exe = os.path.join(REPO, "examples", "guided_hip")
    if not os.path.exists(exe):
        subprocess.run(["make", "-s", "-C", os.path.join(REPO, "examples"), "guided_hip"], check=True)
    n, S, seed, move = 64, 2, 12345, 16
    out = subprocess.run([exe, str(n), str(S), f"lcg:{seed}", str(move), "0.5", "10", "3.0", "0.8", "1"], check=True, timeout=120,
                         capture_output=True, text=True).stdout
    print(out)
    m = re.match(r"(\d+) guided matches of (\d+) x (\d+)\n", out)
    assert m, out
    img = oracle.lcg_image(n, n, seed)
    with pkg.PyramidContext(n, n, S=S) as a, pkg.PyramidContext(n, n, S=S) as b:
        run_chain(a, b, img, np.ascontiguousarray(np.roll(img, move, axis=1)))
        Q, T = raw_described(pkg, a, 0), raw_described(pkg, b, 0)
        a.match_descriptors(b, ratio=0.0)
        a.set_guided_model(shift(move, 0))
        got = run(a, 3.0, ratio=0.8, unique=True)
    assert got.tobytes() == np_guided(Q, T, shift(move, 0), 3.0, 0.8).tobytes()
    assert tuple(int(x) for x in m.groups()) == (len(got), len(Q), len(T)) and len(got) > 0
    fmt = lambda r: "distance %u second %u (%.4f, %.4f) -> (%.4f, %.4f)" % (r["distance"], r["second"], r["qx"], r["qy"], r["tx"], r["ty"])  # noqa: E731
    python_lines = {fmt(r) for r in got}
    lines = re.findall(r"^query (\d+) train (\d+) (distance .*)$", out, re.M)
    assert len(lines) == min(len(got), 8)
    assert [int(i) for i, _, _ in lines] == sorted({int(i) for i, _, _ in lines})  # ascending, unique queries
    for _, _, rest in lines:
        assert rest in python_lines, rest
