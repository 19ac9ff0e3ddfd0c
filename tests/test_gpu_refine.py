"""On-device sub-pixel keypoint refinement (gdp_refine_keypoints) against the numpy float32 oracle of
tests/refine_oracle.py, which implements the rule of include/gdp.h literally.  The result is a
multiset of records and every comparison is of bit patterns.  All cases run on UPLOADED pyramids,
independent of any build kernel, except the C++ example's."""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

from extrema_oracle import (BIG, ODD, F, assert_short_downloads, small_pipeline, denormal_pyramid, normal_pyramid, np_extrema, packed_size, smooth_pyramid,
                            tie_pyramid)
from refine_oracle import (as_multiset, assert_download_order, extrema_records, np_refine, quad_expect, quad_pyramid,
                           records, records_from_set)

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_KINDS = {"normal": normal_pyramid, "tie": tie_pyramid, "smooth": smooth_pyramid}


def bits(x):
    return int(F(x).view(np.uint32))


def same_records(a, b):
    """Two keypoint record arrays, field by field, values by their bits."""
    a, b = np.asarray(a), np.asarray(b)
    return len(a) == len(b) and all(np.array_equal(np.ascontiguousarray(a[f]).view(np.uint8), np.ascontiguousarray(b[f]).view(np.uint8))
                                    for f in ("octave", "scale", "kind", "row", "col", "value"))


@functools.lru_cache(maxsize=None)
def denormal_records():
    return records_from_set(np_extrema(denormal_pyramid(ODD, 2 ** 20), *ODD)[0])


@functools.lru_cache(maxsize=None)
def expected(kind, shape, contrast, edge_ratio):
    """(the oracle's extrema, the oracle's refinement of them) for a shared pyramid."""
    if kind == "denormal":
        src, rec = denormal_pyramid(shape, 2 ** 20), denormal_records()
    else:
        src, rec = _KINDS[kind](shape), extrema_records(kind, shape)
    return rec, np_refine(src, *shape, rec, contrast, edge_ratio)


def source(kind, shape):
    return denormal_pyramid(shape, 2 ** 20) if kind == "denormal" else _KINDS[kind](shape)


# ---------------------------------------------------------------------------------------------
# 1. exact multiset equality with the oracle
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,shape,contrast,edge_ratio", [
    ("smooth", BIG, 0.0, 0.0), ("smooth", BIG, 0.3, 10.0), ("normal", BIG, 0.0, 0.0), ("smooth", ODD, 0.0, 0.0),
    ("tie", BIG, 0.0, 0.0), ("tie", ODD, 0.0, 0.0), ("denormal", ODD, 0.0, 0.0)],
    ids=["smooth-big", "smooth-big-0.3-10", "normal-big", "smooth-odd", "tie-big", "tie-odd", "denormal-odd"])
def test_exact_multiset(pkg, kind, shape, contrast, edge_ratio):
    H, W, S, O = shape
    rec, (want_kept, why) = expected(kind, shape, contrast, edge_ratio)
    with pkg.PyramidContext(H, W, S=S) as ctx:
        assert ctx.O == O
        ctx.upload_pyramid(source(kind, shape))
        ctx.detect_extrema()
        ctx.refine_keypoints(contrast, edge_ratio)  # the same stream, no synchronisation in between
        got = ctx.refined_keypoints(0)
        kp = ctx.keypoints(0)
        assert ctx.refined_count(0) == len(got)
        ctx.refine_keypoints(contrast, edge_ratio)  # the counter is zeroed again
        again = ctx.refined_keypoints(0)
    print(f"{kind} {shape}: {len(kp)} inputs, {len(got)} kept, oracle {len(want_kept)}")
    assert same_records(kp, rec)  # the refinement's inputs are the oracle's
    assert got.dtype == pkg.REFINED_DTYPE
    assert as_multiset(got) == want_kept
    assert_download_order(got)
    assert got.tobytes() == again.tobytes()
    if kind != "denormal":
        assert 0 < len(want_kept) < len(rec)


# ---------------------------------------------------------------------------------------------
# 2. closed form through upload_keypoints
# ---------------------------------------------------------------------------------------------
QS, QROWS, QCOLS = 5, 24, 40
CENTRE = (3.25, 10.125, 20.5)
STARTS = [(3, 10, 20), (5, 10, 20), (1, 14, 17), (3, 10, 21), (3, 12, 24), (3, 10, 25), (3, 10, 26), (3, 16, 20)]


def refine_uploaded(pkg, D, recs, contrast=0.0, edge_ratio=0.0):
    with pkg.PyramidContext(D.shape[1], D.shape[2], S=D.shape[0] - 3, octaves=1) as ctx:
        ctx.upload_pyramid(np.ascontiguousarray(D).ravel())
        ctx.upload_keypoints(recs)
        assert ctx.keypoint_count(0) == len(recs)
        ctx.refine_keypoints(contrast, edge_ratio)
        return ctx.refined_keypoints(0)


def test_eight_starts_closed_form(pkg):
    D = quad_pyramid(QS, QROWS, QCOLS, *CENTRE)
    got = refine_uploaded(pkg, D, records(STARTS))
    expect = []
    for st in STARTS:
        e = quad_expect(st, *CENTRE, QS, QROWS, QCOLS)
        if e:
            (s, r, c), (ds, dr, dc), _ = e
            expect.append((0, s, 1, r, c, int(D[s, r, c].view(np.uint32)), bits(ds), bits(dr), bits(dc), bits(64.0)))
    assert len(expect) == 6 and {t[1:2] + t[3:5] for t in expect} == {(3, 10, 20), (3, 10, 21)}
    assert as_multiset(got) == sorted(expect)
    assert_download_order(got)


def test_kind_is_copied_from_the_input(pkg):
    D = quad_pyramid(QS, QROWS, QCOLS, *CENTRE)
    recs = records(STARTS[:2])
    recs["kind"][1] = -1
    got = refine_uploaded(pkg, D, recs)
    assert sorted(got["kind"].tolist()) == [-1, 1] and set(zip(got["row"].tolist(), got["col"].tolist())) == {(10, 20)}
    assert_download_order(got)  # identical but for the kind: ordered by its bits, +1 (0x01) before -1 (0xff)
    assert got["kind"].tolist() == [1, -1]


def test_mixed_term_against_the_oracle(pkg):
    D = quad_pyramid(QS, QROWS, QCOLS, *CENTRE, mix=0.125)
    starts = [(s, r, c) for s in (2, 3, 4) for r in (8, 10, 13) for c in (17, 20, 21, 24)]
    recs = records(starts)
    want_kept, why = np_refine(D.ravel(), QROWS, QCOLS, QS, 1, recs)
    assert 0 < len(want_kept) <= len(starts) and "ok" in why
    assert as_multiset(refine_uploaded(pkg, D, recs)) == want_kept


@pytest.mark.parametrize("centre", [(3.25, 10.125, -3.0), (3.25, 10.125, QCOLS + 2.0), (3.25, -3.0, 20.5),
                                    (3.25, QROWS + 2.0, 20.5), (-1.0, 10.125, 20.5), (QS + 3.0, 10.125, 20.5)])
def test_peak_outside_a_face_walks_out(pkg, centre):
    D = quad_pyramid(QS, QROWS, QCOLS, *centre)
    starts = [(s, r, c) for s in (1, 2, QS - 1, QS) for r in (1, 2, QROWS - 3, QROWS - 2) for c in (1, 2, QCOLS - 3, QCOLS - 2)]
    assert all(quad_expect(st, *centre, QS, QROWS, QCOLS) is None for st in starts)
    assert len(refine_uploaded(pkg, D, records(starts))) == 0


def test_level_s_plus_2_is_never_read(pkg):
    D = quad_pyramid(QS, QROWS, QCOLS, QS + 0.25, 10.125, 20.5)
    D[QS + 2] = np.nan
    got = refine_uploaded(pkg, D, records([(QS, 10, 20), (QS - 2, 10, 20)]))
    want = (0, QS, 1, 10, 20, int(D[QS, 10, 20].view(np.uint32)), bits(0.25), bits(0.125), bits(0.5), bits(64.0))
    assert as_multiset(got) == [want, want]


def test_contrast_and_edge_thresholds_are_strict(pkg):
    D = quad_pyramid(QS, QROWS, QCOLS, *CENTRE)
    one = records(STARTS[:1])
    assert len(refine_uploaded(pkg, D, one, contrast=63.9375)) == 1  # interp is exactly 64
    assert len(refine_uploaded(pkg, D, one, contrast=64.0)) == 0
    assert len(refine_uploaded(pkg, D, one, edge_ratio=2.0)) == 0  # tr^2 / det = 4.5 = (2+1)^2 / 2
    assert len(refine_uploaded(pkg, D, one, edge_ratio=2.125)) == 1


# ---------------------------------------------------------------------------------------------
# 3. wave and block seams of the compaction
# ---------------------------------------------------------------------------------------------
def test_compaction_seams(pkg):
    D = quad_pyramid(QS, QROWS, QCOLS, *CENTRE)
    want = (0, 3, 1, 10, 20, int(D[3, 10, 20].view(np.uint32)), bits(0.25), bits(0.125), bits(0.5), bits(64.0))
    with pkg.PyramidContext(QROWS, QCOLS, S=QS, octaves=1) as ctx:
        ctx.upload_pyramid(D.ravel())
        for n in (0, 1, 63, 64, 65, 128, 129, 255, 256, 257):
            recs = records([(5, 10, 20) if k % 2 == 0 else (3, 10, 26) for k in range(n)])  # converges / "steps"
            ctx.upload_keypoints(recs)
            ctx.refine_keypoints()
            kept = (n + 1) // 2
            assert ctx.refined_count(0) == kept, n
            assert as_multiset(ctx.refined_keypoints(0)) == [want] * kept, n
        # every lane of some waves rejected, every lane of others kept
        recs = records([(3, 10, 26)] * 64 + [(5, 10, 20)] * 70 + [(3, 10, 26)] * 130 + [(1, 14, 17)] * 3)
        ctx.upload_keypoints(recs)
        ctx.refine_keypoints()
        assert as_multiset(ctx.refined_keypoints(0)) == [want] * 73


# ---------------------------------------------------------------------------------------------
# 4. capacity
# ---------------------------------------------------------------------------------------------
def test_capacity_limits_the_inputs(pkg):
    H, W, S, O = BIG
    with pkg.PyramidContext(H, W, S=S) as ctx:
        ctx.set_keypoint_capacity(100)
        ctx.upload_pyramid(smooth_pyramid(BIG))
        ctx.detect_extrema()
        ctx.refine_keypoints(0.3, 10.0)
        got = ctx.refined_keypoints(0)
        kp = ctx.keypoints(0)
        assert kp.found > 10000 and len(kp) == 100
        want_kept, _ = np_refine(smooth_pyramid(BIG), H, W, S, O, kp, 0.3, 10.0)
        assert ctx.refined_count(0) == len(got) <= 100 and 0 < len(want_kept)
        assert as_multiset(got) == want_kept
        ctx.set_keypoint_capacity(200)  # drops the refined buffer with the keypoint buffer
        assert ctx.refined_count(0) == 0 and len(ctx.refined_keypoints(0)) == 0
        ctx.detect_extrema()
        ctx.refine_keypoints(0.3, 10.0)
        kp = ctx.keypoints(0)
        assert len(kp) == 200
        assert as_multiset(ctx.refined_keypoints(0)) == np_refine(smooth_pyramid(BIG), H, W, S, O, kp, 0.3, 10.0)[0]


# ---------------------------------------------------------------------------------------------
# 5. batch
# ---------------------------------------------------------------------------------------------
def test_batch_images_are_independent(pkg):
    H, W, S, O = ODD
    zeros = np.zeros(packed_size(*ODD), np.float32)
    with pkg.PyramidContext(H, W, S=S, batch=3) as ctx:
        for b, p in enumerate((smooth_pyramid(ODD), zeros, normal_pyramid(ODD))):
            ctx.upload_pyramid(p, b)
        ctx.detect_extrema()
        ctx.refine_keypoints()
        got = [ctx.refined_keypoints(b) for b in range(3)]
        recs = [ctx.device_refined(b)[0] for b in range(3)]
        assert recs[1] - recs[0] == recs[2] - recs[1] == 65536 * 32
    assert as_multiset(got[0]) == expected("smooth", ODD, 0.0, 0.0)[1][0]
    assert len(got[1]) == 0
    assert as_multiset(got[2]) == expected("normal", ODD, 0.0, 0.0)[1][0]
    assert len(got[0]) > 100 and len(got[2]) > 100 and as_multiset(got[0]) != as_multiset(got[2])


# ---------------------------------------------------------------------------------------------
# 6. errors
# ---------------------------------------------------------------------------------------------
def test_refused_contexts_and_arguments(pkg):
    with pkg.PyramidContext(64, 64, S=2, octaves=5, row_begin=0, row_end=32) as ctx:
        with pytest.raises(pkg.GdpError) as e:
            ctx.refine_keypoints()
        assert e.value.status == 3 and "band" in str(e.value)
    with pkg.PyramidContext(64, 64, S=2) as ctx:
        with pytest.raises(pkg.GdpError) as e:  # a fresh context: no keypoint list yet
            ctx.refine_keypoints()
        assert e.value.status == 3
        with pytest.raises(pkg.GdpError) as e:
            ctx.device_refined(0)
        assert e.value.status == 3
        assert ctx.refined_count(0) == 0 and len(ctx.refined_keypoints(0)) == 0
        ctx.set_keypoint_capacity(16)  # a keypoint buffer exists from here on
        for contrast, edge_ratio in [(-1.0, 0.0), (float("nan"), 0.0), (0.0, 0.5), (0.0, float("inf"))]:
            with pytest.raises(pkg.GdpError) as e:
                ctx.refine_keypoints(contrast, edge_ratio)
            assert e.value.status == 1, (contrast, edge_ratio)


def test_upload_keypoints_validates_every_record(pkg):
    S, rows, cols = 2, 16, 24
    good = records([(1, 1, 1), (2, 6, 11), (S, rows - 2, cols - 2)])
    with pkg.PyramidContext(rows, cols, S=S, octaves=2) as ctx:
        ctx.set_keypoint_capacity(8)
        ctx.upload_keypoints(good)
        octave1 = records([(1, 6, 10)], octave=1)  # octave 1 is 8 x 12
        ctx.upload_keypoints(octave1)
        assert same_records(ctx.keypoints(0), octave1)
        ctx.upload_keypoints(good)
        bad = []
        for field, value in [("scale", 0), ("scale", S + 1), ("row", 0), ("row", rows - 1), ("col", 0), ("col", cols - 1),
                             ("octave", 2), ("kind", 0), ("kind", 2)]:
            r = good.copy()
            r[field][1] = value
            bad.append(r)
        r = records([(1, 7, 5)], octave=1)  # row 7 is the last row of octave 1
        bad += [r, np.concatenate([good] * 3)]  # 9 records > the capacity of 8
        for r in bad:
            with pytest.raises(pkg.GdpError) as e:
                ctx.upload_keypoints(r)
            assert e.value.status == 1
            assert ctx.keypoint_count(0) == 3 and same_records(ctx.keypoints(0), good)  # the list is unchanged


# ---------------------------------------------------------------------------------------------
# 7. the C++ example, executed
# ---------------------------------------------------------------------------------------------
def test_cpp_example_matches_the_python_path(pkg, oracle):
    exe = os.path.join(REPO, "examples", "refine_hip")
    if not os.path.exists(exe):
        subprocess.run(["make", "-s", "-C", os.path.join(REPO, "examples"), "refine_hip"], check=True)
    n, S, seed = 64, 2, 12345
    out = subprocess.run([exe, str(n), str(S), f"lcg:{seed}", "0.5", "10"], check=True, timeout=120, capture_output=True,
                         text=True).stdout
    m = re.match(r"(\d+) keypoints, (\d+) refined\n", out)
    assert m, out
    g = pkg.GaussPyramid(oracle.lcg_image(n, n, seed), n, S)
    try:
        g.GenerateDoG()
        kp = g.DetectExtrema()
        rf = g.RefineKeypoints(0.5, 10.0)
        want_kept, _ = np_refine(g.pyramid(), n, n, S, g.layer, kp, 0.5, 10.0)
    finally:
        g.close()
    print(out)
    assert (int(m.group(1)), int(m.group(2))) == (len(kp), len(rf)) and len(kp) > 0
    assert as_multiset(rf) == want_kept
    assert len(re.findall(r"^octave \d+ scale ", out, re.M)) == min(len(rf), 8)


def test_download_through_a_short_buffer_and_through_none(pkg, oracle):
    L = pkg.lib()
    with small_pipeline(pkg, oracle, 2) as ctx:  # gdp_download_refined has no `found`
        assert_short_downloads(lambda host, n, stored, _: L.gdp_download_refined(ctx._ctx, 0, host, n, stored),
                               ctx.refined_keypoints(0), found=False)
