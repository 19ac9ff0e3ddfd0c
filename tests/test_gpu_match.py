"""On-device descriptor matching (gdp_match_descriptors) against the literal numpy oracle of
tests/match_oracle.py.  Distances are exact integers and ties have a total order, so the result is an
exact set: every comparison is equality of the downloaded records' bytes with the oracle's.  The
describe objects of the synthetic cases come from a 40 x 56, S = 2, two-octave context; the lists are
the caller's (gdp_match_set_input) except in the pipeline, two-context, state and example cases."""
import ctypes
import functools
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

from extrema_oracle import ODD, F, assert_short_downloads, small_pipeline, smooth_pyramid
from match_oracle import DESCRIBED_DT, MATCH_DT, NONE, distances, np_match

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# k_match_nn's schedule (csrc/gdp_match.inc): a wave owns 32 queries and sweeps train tiles of 32; the
# train list is cut into chunks whose length is a multiple of CHUNK_UNIT; inside a chunk the packed
# keys are folded at every multiple of WINDOW records
TILE, CHUNK_UNIT, WINDOW = 32, 128, 512
CAPACITY = 1100  # 35 query tiles: 9 chunks of the train list, so 129 records are two chunks, 257 three
SMALL = (0, 1, 2, 31, 32, 33, 63, 64, 65, 97)
SEAMS = ((127, 129), (128, 257), (129, 128), (256, 511), (257, 1025), (513, 256), (1024, 33), (1025, 1023), (33, 1024), (512, 513),
         (255, 255), (2, 127))


def small_context(pkg, capacity=(CAPACITY, CAPACITY)):
    ctx = pkg.PyramidContext(40, 56, S=2, octaves=2)
    ctx.set_match_capacity(*capacity)
    return ctx


def random_records(n, seed):
    """n records of random bytes with plausible positions (finite floats: NaN payloads are not the
    rule's business)."""
    rng = np.random.default_rng(seed)
    R = np.zeros(n, DESCRIBED_DT)
    R["desc"] = rng.integers(0, 256, (n, 128), dtype=np.uint8)
    R["octave"], R["scale"], R["kind"] = rng.integers(0, 40, n), rng.integers(1, 3, n), rng.choice([-1, 1], n)
    R["row"], R["col"] = rng.integers(-5, 4000, n), rng.integers(-5, 4000, n)
    for f in ("value", "dscale", "drow", "dcol", "interp", "angle", "peak"):
        R[f] = rng.uniform(-0.75, 0.75, n).astype(F)
    R["bin"], R["peaks"] = rng.integers(0, 36, n), rng.integers(1, 4, n)
    return R


@functools.lru_cache(maxsize=None)
def list_pair(nq, nt):
    """Random train records; half of the queries are noisy copies of train records (so that the
    ratio and mutual tests keep some and drop some), the rest random."""
    T = random_records(nt, 1000 + nt)
    Q = random_records(nq, 5000 + nq)
    rng = np.random.default_rng(nq * 7919 + nt)
    if nt:
        for i in range(0, nq, 2):
            noise = rng.integers(-12, 13, 128)
            Q["desc"][i] = np.clip(T["desc"][rng.integers(0, nt)].astype(np.int64) + noise, 0, 255)
    Q.setflags(write=False)
    T.setflags(write=False)
    return Q, T, distances(Q, T)


def run(ctx, **kw):
    ctx.match_descriptors(**kw)
    got = ctx.matches()
    assert got.found == ctx.match_count() == len(got)
    return got


def assert_pair(pkg, ctx, Q, T, D=None, what=None):
    """All four combinations of ratio off / 0.8 and mutual off / on, byte for byte."""
    ctx.set_match_input(0, Q)
    ctx.set_match_input(1, T)
    D = distances(Q, T) if D is None else D
    kept = []
    for ratio, mutual in itertools.product((0.0, 0.8), (False, True)):
        got = run(ctx, ratio=ratio, max_distance=None, mutual=mutual)
        want = np_match(Q, T, ratio, NONE, mutual, D=D)
        assert got.dtype == pkg.MATCH_DTYPE
        assert got.tobytes() == want.tobytes(), (what, ratio, mutual, len(got), len(want))
        kept.append(len(want))
    return kept


# ---------------------------------------------------------------------------------------------
# 1. the caller's lists of random bytes: every length at the tile, chunk and window seams
# ---------------------------------------------------------------------------------------------
def test_layout_is_what_the_test_mirrors(pkg):
    with small_context(pkg) as ctx:
        assert ctx.match_layout() == (CAPACITY, CAPACITY, CHUNK_UNIT, 9, 9)
    with small_context(pkg, (140000, CAPACITY)) as ctx:  # 4,375 query tiles: the train list is ONE chunk
        assert ctx.match_layout() == (140000, CAPACITY, CHUNK_UNIT, 1, 118)
    with small_context(pkg, (0, 0)) as ctx:  # 0: the describe object's capacity
        assert ctx.match_layout()[:2] == (2 * 65536, 2 * 65536)


def test_callers_lists_small_lengths(pkg):
    kept = np.zeros(4, np.int64)
    with small_context(pkg) as ctx:
        for nq, nt in itertools.product(SMALL, SMALL):  # nq != nt in 90 of the 100: a swapped axis cannot pass
            kept += assert_pair(pkg, ctx, *list_pair(nq, nt), what=(nq, nt))
    print("kept over the 100 pairs (ratio off/on x mutual off/on):", kept)
    assert kept[0] > kept[1] > 0 and kept[0] > kept[2] > 0 and kept[3] > 0  # every filter keeps some and drops some


@pytest.mark.parametrize("nq,nt", SEAMS)
def test_callers_lists_at_the_chunk_seams(pkg, nq, nt):
    with small_context(pkg) as ctx:
        kept = assert_pair(pkg, ctx, *list_pair(nq, nt), what=(nq, nt))
    assert kept[0] == nq


@pytest.mark.parametrize("nq,nt", [(33, 513), (65, 1025), (2, 1024), (1, 511)])
def test_one_chunk_crosses_the_key_windows(pkg, nq, nt):
    """With 4,375 query tiles in the capacity grid the train list is one chunk, so a wave's sweep
    crosses the 512-record windows of its packed keys and folds them."""
    with small_context(pkg, (140000, CAPACITY)) as ctx:
        kept = assert_pair(pkg, ctx, *list_pair(nq, nt), what=(nq, nt))
    assert kept[0] == nq


# ---------------------------------------------------------------------------------------------
# 2. one-hot lists: A and B must agree on the byte of every K index
# ---------------------------------------------------------------------------------------------
def test_one_hot_k_order(pkg):
    Q, T = np.zeros(128, DESCRIBED_DT), np.zeros(128, DESCRIBED_DT)
    for i in range(128):
        Q["desc"][i, i] = 200
        T["desc"][i, 127 - i] = 180
    with small_context(pkg) as ctx:
        ctx.set_match_input(0, Q)
        ctx.set_match_input(1, T)
        got = run(ctx, ratio=0.0)
    assert list(got["query"]) == list(range(128))
    assert list(got["train"]) == [127 - i for i in range(128)]
    assert (got["distance"] == 400).all() and (got["second"] == 200 * 200 + 180 * 180).all()
    assert got.tobytes() == np_match(Q, T).tobytes()


# ---------------------------------------------------------------------------------------------
# 3. value extremes, at the seams of the ^ 0x80 shift
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("q,t,distance", [(0, 255, 8323200), (255, 255, 0), (128, 127, 128), (127, 128, 128), (255, 0, 8323200)])
def test_value_extremes(pkg, q, t, distance):
    Q, T = random_records(3, 1), random_records(2, 2)
    Q["desc"], T["desc"] = q, t
    with small_context(pkg) as ctx:
        ctx.set_match_input(0, Q)
        ctx.set_match_input(1, T[:1])
        one = run(ctx, ratio=0.0)
        ctx.set_match_input(1, T)
        two = run(ctx, ratio=0.0)
    assert (one["distance"] == distance).all() and (one["second"] == NONE).all() and len(one) == 3  # nt = 1
    assert (two["distance"] == distance).all() and (two["second"] == distance).all() and (two["train"] == 0).all()
    assert one.tobytes() == np_match(Q, T[:1]).tobytes() and two.tobytes() == np_match(Q, T).tobytes()


# ---------------------------------------------------------------------------------------------
# 4. ties: the lowest index wins, second == distance, mutual keeps the lowest duplicate query
# ---------------------------------------------------------------------------------------------
def test_ties_go_to_the_lowest_index(pkg):
    rng = np.random.default_rng(11)
    base = random_records(100, 3)
    where = rng.permutation(300)  # train record k is base[where[k] % 100]: three copies, scattered over three chunks
    T = base[where % 100].copy()
    Q = np.concatenate([base, base[rng.permutation(100)]])  # every query twice
    lowest_train = {b: min(k for k in range(300) if where[k] % 100 == b) for b in range(100)}
    with small_context(pkg) as ctx:
        assert ctx.match_layout()[3] == 9  # 300 records: chunks of 128
        ctx.set_match_input(0, Q)
        ctx.set_match_input(1, T)
        got = run(ctx, ratio=0.0)
        mutual = run(ctx, ratio=0.0, mutual=True)
    assert len(got) == 200 and (got["distance"] == 0).all() and (got["second"] == 0).all()
    assert [int(j) for j in got["train"][:100]] == [lowest_train[b] for b in range(100)]
    # the copies of a record lie in different chunks, and so do the winners (the lowest copies crowd the first two)
    assert sum(len({k // CHUNK_UNIT for k in range(300) if where[k] % 100 == b}) > 1 for b in range(100)) > 50
    assert len({k // CHUNK_UNIT for k in lowest_train.values()}) >= 2
    D = distances(Q, T)
    assert got.tobytes() == np_match(Q, T, D=D).tobytes() and mutual.tobytes() == np_match(Q, T, mutual=True, D=D).tobytes()
    # of the two copies of a query only the lowest is the nearest query of its train record
    assert len(mutual) == 100 and all(int(i) == min(k for k in range(200) if Q["desc"][k].tobytes() == Q["desc"][i].tobytes())
                                      for i in mutual["query"])


# ---------------------------------------------------------------------------------------------
# 5. filter seams: (float)distance == r2 * (float)second, and max_distance == distance
# ---------------------------------------------------------------------------------------------
def test_filter_seams(pkg):
    def ones(k):
        r = random_records(1, k)
        r["desc"] = 0
        r["desc"][0, :k] = 1
        return r

    Q = ones(0)
    with small_context(pkg) as ctx:
        ctx.set_match_input(0, Q)
        seen = set()
        for distance, second, ratio in ((16, 25, 0.8), (25, 100, 0.5), (64, 100, 0.8), (9, 25, 0.6), (36, 100, 0.6), (1, 4, 0.5),
                                        (49, 100, 0.7), (16, 25, 0.81), (16, 25, 0.79)):
            T = np.concatenate([ones(second), ones(distance)])  # the nearest is train 1
            ctx.set_match_input(1, T)
            want = np_match(Q, T, ratio)
            got = run(ctx, ratio=ratio)
            r2 = F(ratio) * F(ratio)
            print(f"distance {distance} second {second} ratio {ratio}: r2 * second = {float(r2 * F(second))!r}: kept {len(want)}")
            assert got.tobytes() == want.tobytes(), (distance, second, ratio)
            seen.add(len(want))
            if len(got):
                assert (int(got["train"][0]), int(got["distance"][0]), int(got["second"][0])) == (1, distance, second)
            assert len(run(ctx, ratio=0.0, max_distance=distance)) == 1  # the cap is inclusive
            assert len(run(ctx, ratio=0.0, max_distance=distance - 1)) == 0
            assert len(run(ctx, ratio=0.0, max_distance=0xFFFFFFFF)) == 1
        assert seen == {0, 1}


# ---------------------------------------------------------------------------------------------
# 6. the pipeline on one stream, image 0 against image 1 of a batch of two
# ---------------------------------------------------------------------------------------------
def raw_described(pkg, ctx, b):
    """Image b's described list in DEVICE order: the order the match's indices name (test plumbing)."""
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    ctx.sync()
    out = np.zeros(ctx.described_count(b), pkg.DESCRIBED_DTYPE)
    assert hip.hipMemcpy(out.ctypes.data, ctx.device_described(b)[0], out.nbytes, 2) == 0  # hipMemcpyDeviceToHost (synchronous)
    return out


@functools.lru_cache(maxsize=None)
def variant_pyramid():
    """smooth_pyramid(ODD) dimmed and slightly disturbed: nearly the same keypoints and descriptors."""
    p = smooth_pyramid(ODD)
    rng = np.random.default_rng(17)
    v = (p * F(0.9) + rng.standard_normal(p.shape).astype(F) * F(0.02) * p.std()).astype(F)
    v.setflags(write=False)
    return v


def chain(ctx):
    ctx.detect_extrema()
    ctx.refine_keypoints()
    ctx.orient_keypoints()
    ctx.describe_keypoints()


def test_pipeline_on_one_stream(pkg):
    H, W, S, O = ODD
    with pkg.PyramidContext(H, W, S=S, batch=2) as ctx:
        ctx.upload_pyramid(smooth_pyramid(ODD), 0)
        ctx.upload_pyramid(variant_pyramid(), 1)
        chain(ctx)
        ctx.match_descriptors(query_image=0, train_image=1, ratio=0.8)  # the same stream, no synchronisation in between
        got = ctx.matches()
        Q, T = raw_described(pkg, ctx, 0), raw_described(pkg, ctx, 1)
        ctx.match_descriptors(query_image=0, train_image=1, ratio=0.8)  # the counter is zeroed again
        again = ctx.matches()
        D = distances(Q, T)
        want = np_match(Q, T, 0.8, D=D)
        print(f"{len(Q)} x {len(T)} described records: {len(want)} matches at ratio 0.8")
        assert len(Q) > 500 and len(T) > 0
        assert got.tobytes() == want.tobytes() == again.tobytes()
        assert run(ctx, query_image=1, train_image=0, ratio=0.8, mutual=True).tobytes() == np_match(T, Q, 0.8, mutual=True).tobytes()
        assert run(ctx, query_image=1, train_image=1, ratio=0.0, max_distance=0).tobytes() == np_match(T, T, 0.0, 0).tobytes()
        own = random_records(40, 9)  # a caller's list on the train side, then back to the described list
        ctx.set_match_input(1, own)
        assert run(ctx, query_image=0, train_image=1, ratio=0.0).tobytes() == np_match(Q, own).tobytes()
        ctx.set_match_input(1, None)
        assert run(ctx, query_image=0, train_image=1, ratio=0.8).tobytes() == want.tobytes()


# ---------------------------------------------------------------------------------------------
# 7. two contexts of different geometry
# ---------------------------------------------------------------------------------------------
def test_two_contexts_of_different_geometry(pkg, oracle):
    with pkg.PyramidContext(64, 64, S=2) as a, pkg.PyramidContext(48, 80, S=3) as b:
        for ctx, seed in ((a, 12345), (b, 777)):
            ctx.set_input(oracle.lcg_image(ctx.H, ctx.W, seed))
            ctx.build_gaussian()
            ctx.detect_extrema()
            ctx.refine_keypoints(0.5, 10.0)
            ctx.orient_keypoints()
            ctx.describe_keypoints()
        Q, T = raw_described(pkg, a, 0), raw_described(pkg, b, 0)  # synchronises both contexts' streams
        a.match_descriptors(b, ratio=0.9, mutual=True)
        got = a.matches()
        assert 0 < len(Q) != len(T) > 0
        assert got.tobytes() == np_match(Q, T, 0.9, mutual=True).tobytes()
        b.match_descriptors(a, ratio=0.0)  # the other direction, an object of b's
        assert b.matches().tobytes() == np_match(T, Q).tobytes() and b.match_count() == len(T)
        a.match_descriptors(ratio=0.0, max_distance=0)  # train None: a against itself, a new object
        assert list(a.matches()["train"]) == list(np_match(Q, Q, 0.0, 0)["train"])
    # both contexts are closed: the match objects went before the describe objects they read


# ---------------------------------------------------------------------------------------------
# 8. state: matching only reads the contexts, the orientation and the describe objects
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
        state = lambda: (ctx.checksum(0), ctx.keypoints(0).tobytes(), ctx.refined_keypoints(0).tobytes(),  # noqa: E731
                         ctx.oriented_keypoints(0).tobytes(), ctx.described_keypoints(0).tobytes(), ctx.pyramid(0).tobytes())
        before = state()
        Q = raw_described(pkg, ctx, 0)
        got = run(ctx, ratio=0.8, mutual=True)
        assert ctx.tuning()["zeros_clean"] == 1  # the next build is still the steady-state one
        assert state() == before and len(before[4]) > 0
        assert got.tobytes() == np_match(Q, Q, 0.8, mutual=True).tobytes() and len(got) > 0
        ctx.build()
        assert ctx.tuning()["zeros_clean"] == 1 and ctx.checksum(0) == before[0]
        assert run(ctx, ratio=0.8, mutual=True).tobytes() == got.tobytes()


# ---------------------------------------------------------------------------------------------
# 9. refusals
# ---------------------------------------------------------------------------------------------
def test_refusals(pkg):
    Q, T, D = list_pair(33, 65)
    with small_context(pkg, (40, 70)) as ctx:
        ctx.set_match_input(0, Q)
        ctx.set_match_input(1, T)
        want = np_match(Q, T, 0.8, D=D)
        assert run(ctx, ratio=0.8).tobytes() == want.tobytes()
        for ratio in (float("nan"), -0.5, 1.5, float("inf"), -0.0 - 1e-30):
            with pytest.raises(pkg.GdpError) as e:
                ctx.match_descriptors(ratio=ratio)
            assert e.value.status == 1 and "ratio" in str(e.value)
        for kw in ({"query_image": 1}, {"train_image": 1}, {"query_image": -1}, {"train_image": -1}):
            with pytest.raises(pkg.GdpError) as e:
                ctx.match_descriptors(ratio=0.8, **kw)
            assert e.value.status == 1
        for side, n in ((0, 41), (1, 71)):  # a list above that side's capacity
            with pytest.raises(pkg.GdpError) as e:
                ctx.set_match_input(side, random_records(n, 4))
            assert e.value.status == 1 and "capacity" in str(e.value)
        with pytest.raises(pkg.GdpError):
            ctx.set_match_input(2, Q)
        ctx.match_descriptors(ratio=1.0)  # the closed end of (0, 1]
        assert ctx.matches().tobytes() == np_match(Q, T, 1.0, D=D).tobytes()
        # nothing above changed the lists: the previous ones still stand
        assert run(ctx, ratio=0.8).tobytes() == want.tobytes()
        ctx.set_match_input(0, random_records(40, 5))  # exactly the capacity is fine
        assert len(run(ctx, ratio=0.0)) == 40


def test_objects_on_different_devices_are_refused(pkg):
    if pkg.lib().gdp_device_count() < 2:
        pytest.skip("needs two devices")
    with pkg.PyramidContext(40, 56, S=2, octaves=2, device=0) as a, pkg.PyramidContext(40, 56, S=2, octaves=2, device=1) as b:
        with pytest.raises(pkg.GdpError) as e:
            a.match_descriptors(b)
        assert e.value.status == 1 and "device" in str(e.value)


# ---------------------------------------------------------------------------------------------
# 10. the C++ example, executed
# ---------------------------------------------------------------------------------------------
def test_cpp_example_matches_the_python_path(pkg, oracle):
    """Two 64 x 64 LCG images, the second moved 16 columns to the right.  The described lists'
    device order, which the indices name, depends on the waves' timing and so may differ between the
    two processes: the counts must be equal, and each of the example's first eight lines, without
    its two indices, must be a record of the Python path."""
    exe = os.path.join(REPO, "examples", "match_hip")
    if not os.path.exists(exe):
        subprocess.run(["make", "-s", "-C", os.path.join(REPO, "examples"), "match_hip"], check=True)
    n, S, seed, shift = 64, 2, 12345, 16
    out = subprocess.run([exe, str(n), str(S), f"lcg:{seed}", str(shift), "0.5", "10", "0.8", "1"], check=True, timeout=120,
                         capture_output=True, text=True).stdout
    print(out)
    m = re.match(r"(\d+) matches of (\d+) x (\d+)\n", out)
    assert m, out
    img = oracle.lcg_image(n, n, seed)
    with pkg.PyramidContext(n, n, S=S) as a, pkg.PyramidContext(n, n, S=S) as b:
        for ctx, image in ((a, img), (b, np.roll(img, shift, axis=1))):
            ctx.set_input(np.ascontiguousarray(image))
            ctx.build_gaussian()
            ctx.detect_extrema()
            ctx.refine_keypoints(0.5, 10.0)
            ctx.orient_keypoints()
            ctx.describe_keypoints()
        Q, T = raw_described(pkg, a, 0), raw_described(pkg, b, 0)
        a.match_descriptors(b, ratio=0.8, mutual=True)
        got = a.matches()
    assert got.tobytes() == np_match(Q, T, 0.8, mutual=True).tobytes()
    assert tuple(int(x) for x in m.groups()) == (len(got), len(Q), len(T)) and len(got) > 0
    fmt = lambda r: "distance %u second %u (%.4f, %.4f) -> (%.4f, %.4f)" % (r["distance"], r["second"], r["qx"], r["qy"], r["tx"], r["ty"])  # noqa: E731
    python_lines = {fmt(r) for r in got}
    lines = re.findall(r"^query (\d+) train (\d+) (distance .*)$", out, re.M)
    assert len(lines) == min(len(got), 8)
    assert [int(q) for q, _, _ in lines] == sorted({int(q) for q, _, _ in lines})  # ascending, unique queries
    for _, _, rest in lines:
        assert rest in python_lines, rest
    moved = np.count_nonzero((got["tx"] - got["qx"] == F(shift)) & (got["ty"] - got["qy"] == 0))
    print(f"{moved} of {len(got)} kept matches are displaced by exactly ({shift}, 0)")  # reported, not asserted


# ---------------------------------------------------------------------------------------------
# 11. the list handling's edges on the small image: lists just over one 32-record tile
# ---------------------------------------------------------------------------------------------
def test_short_downloads_and_an_empty_list_then_none(pkg, oracle):
    L = pkg.lib()
    Q, T, D = list_pair(33, 40)
    with small_pipeline(pkg, oracle, 4) as ctx:
        before = run(ctx, ratio=0.0)  # both sides read the described list
        assert len(before) == ctx.described_count(0) > 0
        ctx.set_match_input(0, Q)
        ctx.set_match_input(1, T)
        full = run(ctx, ratio=0.0)
        assert full.tobytes() == np_match(Q, T, 0.0, D=D).tobytes() and len(full) == 33
        assert_short_downloads(lambda *a: L.gdp_download_matches(ctx._match, *a), full)
        ctx.set_match_input(0, Q[:0])
        assert len(run(ctx, ratio=0.0)) == 0
        for side in (0, 1):
            ctx.set_match_input(side, None)  # the described list again
        assert run(ctx, ratio=0.0).tobytes() == before.tobytes()
