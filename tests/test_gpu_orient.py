"""On-device keypoint orientation (gdp_orient_keypoints) against the numpy float32 oracle of
tests/orient_oracle.py, which implements the rule of include/gdp.h literally.  The result is a
multiset of 48-byte records and every comparison is of bit patterns.  The oracle is handed the
LIBRARY's weight tables (glibc expf and numpy may differ in the last bit).  All cases run on UPLOADED
pyramids, independent of any build kernel, except the state test's and the C++ example's."""
import collections
import functools
import os
import re
import subprocess

import numpy as np
import pytest

from extrema_oracle import (BIG, ODD, F, assert_short_downloads, denormal_pyramid, normal_pyramid, np_extrema, small_pipeline,
                            smooth_pyramid, tie_pyramid)
from orient_oracle import (DIRECTIONS, as_multiset, assert_download_order, gradient_pyramid, np_orient, refined_from,
                           refined_records)
from refine_oracle import extrema_records, records_from_set

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_KINDS = {"normal": normal_pyramid, "tie": tie_pyramid, "smooth": smooth_pyramid}
_TABLES = {}


def bits(x):
    return int(F(x).view(np.uint32))


def tables(pkg, S):
    """{s: the library's w_s}: what the kernel was given."""
    if S not in _TABLES:
        _TABLES[S] = {s: pkg.orient_weights(S, s)[0] for s in range(1, S + 1)}
    return _TABLES[S]


def source(kind, shape):
    return denormal_pyramid(shape, 2 ** 20) if kind == "denormal" else _KINDS[kind](shape)


@functools.lru_cache(maxsize=None)
def oracle_inputs(kind, shape):
    """The oracle's extrema of a shared pyramid as refined records (offsets zero): inputs that do not
    depend on k_extrema or k_refine."""
    if kind == "denormal":
        return refined_from(records_from_set(np_extrema(denormal_pyramid(shape, 2 ** 20), *shape)[0]))
    return refined_from(extrema_records(kind, shape))


@functools.lru_cache(maxsize=None)
def sample(kind, shape, n, seed):
    """A seeded sample of n of the oracle's keypoints: every one of octaves >= 4 (a few dozen, which a
    uniform draw would miss), the rest drawn uniformly from the others."""
    rec = oracle_inputs(kind, shape)
    rare = np.nonzero(rec["octave"] >= 4)[0] if n >= 1000 else np.zeros(0, np.int64)
    rest = np.setdiff1d(np.arange(len(rec)), rare)
    pick = np.sort(np.concatenate([rare, np.random.default_rng(seed).choice(rest, n - len(rare), replace=False)]))
    out = rec[pick]
    out["dscale"], out["drow"], out["dcol"], out["interp"] = 0.25, -0.125, 0.5, 2.5  # copied through
    out.setflags(write=False)
    return out


def orient_inputs(pkg, packed, shape, recs, octaves=0):
    H, W, S, O = shape
    with pkg.PyramidContext(H, W, S=S, octaves=octaves) as ctx:
        ctx.upload_pyramid(packed)
        ctx.set_orient_input(recs)
        ctx.orient_keypoints()
        got = ctx.oriented_keypoints(0)
        assert got.found == ctx.oriented_count(0) == len(got)
        return got


# ---------------------------------------------------------------------------------------------
# 1. the whole pipeline on one stream: exact multiset equality with the oracle
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["smooth", "tie", "denormal"])
def test_pipeline_exact_multiset(pkg, kind):
    H, W, S, O = ODD
    src = source(kind, ODD)
    with pkg.PyramidContext(H, W, S=S) as ctx:
        assert ctx.O == O
        ctx.upload_pyramid(src)
        ctx.detect_extrema()
        ctx.refine_keypoints()
        ctx.orient_keypoints()  # the same stream, no synchronisation in between
        got = ctx.oriented_keypoints(0)
        refined = ctx.refined_keypoints(0)
        ctx.orient_keypoints()  # the counter is zeroed again
        again = ctx.oriented_keypoints(0)
        # the oracle's own extrema as the caller's list: clipped windows and rejection, whatever k_refine kept
        ctx.set_orient_input(oracle_inputs(kind, ODD))
        ctx.orient_keypoints()
        direct = ctx.oriented_keypoints(0)
        ctx.set_orient_input(None)  # back to the context's list
        ctx.orient_keypoints()
        back = ctx.oriented_keypoints(0)
    clipped = []
    want, why = np_orient(src, H, W, S, O, refined, tables(pkg, S))
    want_direct, why_direct = np_orient(src, H, W, S, O, oracle_inputs(kind, ODD), tables(pkg, S), clipped_out=clipped)
    print(f"{kind}: {len(refined)} refined -> {len(got)} oriented (oracle {len(want)}); {len(oracle_inputs(kind, ODD))} extrema "
          f"-> {len(direct)} (oracle {len(want_direct)}), {why_direct.count('nonfinite')} rejected, {sum(clipped)} clipped")
    assert got.dtype == pkg.ORIENTED_DTYPE
    assert as_multiset(got) == want and got.found == len(want)
    assert as_multiset(direct) == want_direct and direct.found == len(want_direct)
    assert_download_order(got)
    assert_download_order(direct)
    assert got.tobytes() == again.tobytes() == back.tobytes()  # repeatable, byte for byte
    if kind == "smooth":
        assert len(want) > len(refined) > 500 and sum(clipped) > 100 and {t[0] for t in want_direct} >= {0, 1, 2, 3}
    if kind == "tie":
        assert why_direct.count("nonfinite") > 50 and 0 < len(want_direct)
    if kind == "denormal":
        assert len(oracle_inputs(kind, ODD)) > 500 and want_direct == []  # gx*gx underflows to +0: flat windows


# ---------------------------------------------------------------------------------------------
# 2. every octave, R = 5 and R = 3: samples of the oracle's keypoints through set_orient_input
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["smooth", "normal"])
def test_sampled_keypoints_of_the_big_pyramids(pkg, kind):
    H, W, S, O = BIG
    recs = sample(kind, BIG, 2000, 5)
    got = orient_inputs(pkg, source(kind, BIG), BIG, recs)
    want, why = np_orient(source(kind, BIG), H, W, S, O, recs, tables(pkg, S))
    print(f"{kind} BIG: 2000 inputs -> {len(got)} oriented, oracle {len(want)}, peaks per input up to {max(t[13] for t in want)}")
    # every octave that has keypoints (octave 6 is 3 x 8, octave 7 has no candidates), R = 5 and R = 3
    assert {int(o) for o in recs["octave"]} >= set(range(6)) and {int(s) for s in recs["scale"]} == {1, 2}
    assert why == ["ok"] * 2000 and len(want) > 2400
    assert as_multiset(got) == want
    assert_download_order(got)
    assert all(t[6:10] == (bits(0.25), bits(-0.125), bits(0.5), bits(2.5)) for t in as_multiset(got))  # copied, not read


# ---------------------------------------------------------------------------------------------
# 3. group, wave and block tails of the list
# ---------------------------------------------------------------------------------------------
def test_list_lengths_at_the_group_wave_and_block_seams(pkg):
    H, W, S, O = ODD
    recs = sample("smooth", ODD, 257, 9)
    want_all, _ = np_orient(smooth_pyramid(ODD), H, W, S, O, recs, tables(pkg, S))
    key = lambda r: (int(r["octave"]), int(r["scale"]), int(r["kind"]), int(r["row"]), int(r["col"]))  # noqa: E731
    with pkg.PyramidContext(H, W, S=S) as ctx:
        ctx.upload_pyramid(smooth_pyramid(ODD))
        for n in (1, 3, 4, 5, 63, 64, 65, 257):
            ctx.set_orient_input(recs[:n])
            ctx.orient_keypoints()
            first = {key(r) for r in recs[:n]}
            want = [t for t in want_all if t[:5] in first]  # positions are unique: the outputs of the first n inputs
            got = ctx.oriented_keypoints(0)
            assert len(want) >= n and as_multiset(got) == want, n
        ctx.set_orient_input(recs[:0])  # an empty list is a list, not the context's
        ctx.orient_keypoints()
        assert ctx.oriented_count(0) == 0 and len(ctx.oriented_keypoints(0)) == 0


# ---------------------------------------------------------------------------------------------
# 4. closed form: constant gradients, and NaN in every level below s
# ---------------------------------------------------------------------------------------------
GS, GROWS, GCOLS = 3, 24, 40


def test_closed_form_directions(pkg):
    shape = (GROWS, GCOLS, GS, 1)
    with pkg.PyramidContext(GROWS, GCOLS, S=GS, octaves=1) as ctx:
        for s in (1, 2, 3):
            recs = refined_records([(s, 12, 20), (s, 1, 1), (s, GROWS - 2, GCOLS - 2)])
            ctx.set_orient_input(recs)
            for (a, b), want_bin in DIRECTIONS:
                D = gradient_pyramid(GS, GROWS, GCOLS, s, a, b)  # levels below s are NaN: reading one rejects everything
                ctx.upload_pyramid(D.ravel())
                ctx.orient_keypoints()
                got = ctx.oriented_keypoints(0)
                want, why = np_orient(D.ravel(), *shape, recs, tables(pkg, GS))
                assert why == ["ok"] * 3
                assert len(got) == 3, (s, a, b)
                assert got["peaks"].tolist() == [1, 1, 1] and got["bin"].tolist() == [want_bin] * 3, (s, a, b)
                assert got["angle"].view(np.uint32).tolist() == [bits(10.0 * want_bin)] * 3, (s, a, b)
                assert sorted(zip(got["row"].tolist(), got["col"].tolist())) == [(1, 1), (12, 20), (GROWS - 2, GCOLS - 2)]
                assert as_multiset(got) == want  # `peak` included
                assert got["value"].tolist() == [1.5] * 3 and got["interp"].tolist() == [2.5] * 3


# ---------------------------------------------------------------------------------------------
# 5. batch: the images' lists are independent, the caller's and the context's side by side
# ---------------------------------------------------------------------------------------------
def test_batch_with_different_lists_per_image(pkg):
    H, W, S, O = ODD
    own = sample("normal", ODD, 100, 3)
    with pkg.PyramidContext(H, W, S=S, batch=2) as ctx:
        ctx.upload_pyramid(smooth_pyramid(ODD), 0)
        ctx.upload_pyramid(normal_pyramid(ODD), 1)
        ctx.detect_extrema()
        ctx.refine_keypoints()
        ctx.set_orient_input(own, b=1)  # image 0 keeps the context's refined list
        ctx.orient_keypoints()
        got = [ctx.oriented_keypoints(b) for b in range(2)]
        refined0 = ctx.refined_keypoints(0)
        addr = [ctx.device_oriented(b)[0] for b in range(2)]
        assert addr[1] - addr[0] == 2 * 65536 * 48  # capacity 0: twice the keypoint capacity
    assert as_multiset(got[0]) == np_orient(smooth_pyramid(ODD), H, W, S, O, refined0, tables(pkg, S))[0]
    assert as_multiset(got[1]) == np_orient(normal_pyramid(ODD), H, W, S, O, own, tables(pkg, S))[0]
    assert len(got[0]) > 500 and len(got[1]) >= 100


# ---------------------------------------------------------------------------------------------
# 6. capacity: the counter counts everything, the buffer holds true records only
# ---------------------------------------------------------------------------------------------
def test_capacity_of_eight(pkg):
    H, W, S, O = ODD
    with pkg.PyramidContext(H, W, S=S) as ctx:
        ctx.set_orient_capacity(8)
        ctx.upload_pyramid(smooth_pyramid(ODD))
        ctx.detect_extrema()
        ctx.refine_keypoints()
        ctx.orient_keypoints()
        got = ctx.oriented_keypoints(0)
        refined = ctx.refined_keypoints(0)
        with pytest.raises(pkg.GdpError) as e:  # the caller's lists are bounded by the same capacity
            ctx.set_orient_input(sample("smooth", ODD, 9, 1))
        assert e.value.status == 1
    want, _ = np_orient(smooth_pyramid(ODD), H, W, S, O, refined, tables(pkg, S))
    assert got.found == len(want) > 800 and len(got) == 8
    assert not collections.Counter(as_multiset(got)) - collections.Counter(want)  # each stored record is a true one
    assert_download_order(got)


# ---------------------------------------------------------------------------------------------
# 7. state: the orientation only reads the context
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
        before = (ctx.checksum(0), ctx.keypoints(0).tobytes(), ctx.refined_keypoints(0).tobytes(), ctx.pyramid(0).tobytes())
        ctx.orient_keypoints()
        got = ctx.oriented_keypoints(0)
        assert ctx.tuning()["zeros_clean"] == 1  # the next build is still the steady-state one
        after = (ctx.checksum(0), ctx.keypoints(0).tobytes(), ctx.refined_keypoints(0).tobytes(), ctx.pyramid(0).tobytes())
        assert before == after and len(before[2]) > 0
        want, _ = np_orient(ctx.pyramid(0), n, n, S, ctx.O, ctx.refined_keypoints(0), tables(pkg, S))
        assert as_multiset(got) == want and len(want) > 0
        ctx.set_keypoint_capacity(4096)  # the context's lists move; the object looks them up at launch
        assert ctx.tuning()["zeros_clean"] == 1
        ctx.detect_extrema()
        ctx.refine_keypoints(0.5, 10.0)
        ctx.orient_keypoints()
        assert ctx.oriented_keypoints(0).tobytes() == got.tobytes()
        ctx.build()
        assert ctx.tuning()["zeros_clean"] == 1 and ctx.checksum(0) == before[0]


# ---------------------------------------------------------------------------------------------
# 8. errors
# ---------------------------------------------------------------------------------------------
def test_refused_contexts_and_inputs(pkg):
    with pkg.PyramidContext(64, 64, S=2, octaves=5, row_begin=0, row_end=32) as ctx:
        with pytest.raises(pkg.GdpError) as e:
            ctx.orient_keypoints()
        assert e.value.status == 3 and "band" in str(e.value)
    S, rows, cols = 2, 16, 24
    good = refined_records([(1, 1, 1), (2, 6, 11), (S, rows - 2, cols - 2)])
    with pkg.PyramidContext(rows, cols, S=S, octaves=2) as ctx:
        with pytest.raises(pkg.GdpError) as e:  # a fresh context: neither a refined buffer nor a list of the caller's
            ctx.orient_keypoints()
        assert e.value.status == 3
        assert ctx.oriented_count(0) == 0 and len(ctx.oriented_keypoints(0)) == 0
        ctx.upload_pyramid(np.zeros(ctx.packed_floats(), np.float32))
        ctx.set_orient_input(good)
        ctx.orient_keypoints()  # a list of the caller's is enough
        assert ctx.oriented_count(0) == 0  # flat windows: no peaks
        bad = []
        for field, value in [("scale", 0), ("scale", S + 1), ("row", 0), ("row", rows - 1), ("col", 0), ("col", cols - 1),
                             ("octave", 2), ("kind", 0)]:
            r = good.copy()
            r[field][1] = value
            bad.append(r)
        bad.append(refined_records([(1, 7, 5)], octave=1))  # row 7 is the last row of octave 1 (8 x 12)
        for r in bad:
            with pytest.raises(pkg.GdpError) as e:
                ctx.set_orient_input(r)
            assert e.value.status == 1
        ctx.set_orient_input(None)  # back to the context's list, which still does not exist
        with pytest.raises(pkg.GdpError) as e:
            ctx.orient_keypoints()
        assert e.value.status == 3


# ---------------------------------------------------------------------------------------------
# 9. the C++ example, executed
# ---------------------------------------------------------------------------------------------
def test_cpp_example_matches_the_python_path(pkg, oracle):
    exe = os.path.join(REPO, "examples", "orient_hip")
    if not os.path.exists(exe):
        subprocess.run(["make", "-s", "-C", os.path.join(REPO, "examples"), "orient_hip"], check=True)
    n, S, seed = 64, 2, 12345
    out = subprocess.run([exe, str(n), str(S), f"lcg:{seed}", "0.5", "10"], check=True, timeout=120, capture_output=True,
                         text=True).stdout
    m = re.match(r"(\d+) keypoints, (\d+) refined, (\d+) oriented\n", out)
    assert m, out
    g = pkg.GaussPyramid(oracle.lcg_image(n, n, seed), n, S)
    try:
        g.GenerateDoG()
        kp = g.DetectExtrema()
        rf = g.RefineKeypoints(0.5, 10.0)
        ok = g.OrientKeypoints()
        want, _ = np_orient(g.pyramid(), n, n, S, g.layer, rf, tables(pkg, S))
    finally:
        g.close()
    print(out)
    assert tuple(int(x) for x in m.groups()) == (len(kp), len(rf), len(ok)) and len(ok) >= len(rf) > 0
    assert as_multiset(ok) == want
    lines = re.findall(r"^octave (\d+) scale (\d+) sample \((\d+), (\d+)\) .* angle (\S+) bin (\d+) of (\d+) ", out, re.M)
    assert len(lines) == min(len(ok), 8)
    for line, k in zip(lines, ok):
        assert line == (str(k["octave"]), str(k["scale"]), str(k["row"]), str(k["col"]), "%.4f" % k["angle"], str(k["bin"]),
                        str(k["peaks"]))


# ---------------------------------------------------------------------------------------------
# 10. the list handling's edges on the small image
# ---------------------------------------------------------------------------------------------
def test_short_downloads_and_an_empty_list_then_none(pkg, oracle):
    L = pkg.lib()
    with small_pipeline(pkg, oracle, 3) as ctx:
        full = ctx.oriented_keypoints(0)
        assert_short_downloads(lambda *a: L.gdp_download_oriented(ctx._orient, 0, *a), full)
        ctx.set_orient_input(np.zeros(0, pkg.REFINED_DTYPE))
        ctx.orient_keypoints()
        assert ctx.oriented_count(0) == 0 and len(ctx.oriented_keypoints(0)) == 0
        ctx.set_orient_input(None)  # the refined list again
        ctx.orient_keypoints()
        assert ctx.oriented_keypoints(0).tobytes() == full.tobytes()
