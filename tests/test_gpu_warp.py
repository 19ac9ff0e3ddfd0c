"""On-device homography warp (gdp_warp_image) against the literal numpy oracle of tests/warp_oracle.py.
The matrix is separately rounded float64, the sampling separately rounded float32 with correctly
rounded divisions, and the statistics are integer sums, so the result is exact: every comparison is
equality of the downloaded image's bytes and of the whole 64-byte record with the oracle's.  A query
context of 40 x 56 and a train context of 48 x 72 (S = 2, two octaves) are used unless a case says
otherwise: different sizes catch H / W and source / destination swaps."""
import ctypes
import functools
import os
import re
import subprocess

import numpy as np
import pytest

from ransac_oracle import NONE
from test_gpu_match import chain
from test_gpu_ransac import raw_matches
from warp_oracle import INT32_MAX, INT32_MIN, WARP_DT, np_warp, np_warp_model

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
QH, QW, TH, TW = 40, 56, 48, 72
DT = {"i32": np.int32, "u8": np.uint8}
IDENTITY = np.eye(3, dtype=F)
ROTATION = np.array([[0.92, -0.31, 9.5], [0.28, 0.95, -4.25], [1e-3, -2e-3, 1.0]], F)


def shift(dx, dy):
    """h taking query (x, y) to train (x + dx, y + dy)."""
    return np.array([[1, 0, dx], [0, 1, dy], [0, 0, 1]], F)


@functools.lru_cache(maxsize=None)
def image(h, w, fmt, seed, wide=False):
    """Random pixels: 8-bit values, or (wide, int32 only) the whole int32 range."""
    rng = np.random.default_rng(1000 * seed + h + w)
    img = rng.integers(INT32_MIN, INT32_MAX + 1, (h, w)).astype(np.int32) if wide else rng.integers(0, 256, (h, w)).astype(DT[fmt])
    img.setflags(write=False)
    return img


def pair(pkg, qfmt="i32", tfmt="i32", qshape=(QH, QW), tshape=(TH, TW), batch=1):
    """(query context, train context) with the match object between them (on two empty lists)."""
    q = pkg.PyramidContext(*qshape, S=2, octaves=min(2, pkg.octaves_for(min(qshape))), batch=batch, input_format=qfmt)
    t = pkg.PyramidContext(*tshape, S=2, octaves=min(2, pkg.octaves_for(min(tshape))), batch=batch, input_format=tfmt)
    for ctx in (q, t):  # no keypoints here: small lists keep the objects between the contexts and the warp light
        ctx.set_keypoint_capacity(64)
    q.match_descriptors(t, ratio=0.0)
    return q, t


def assert_same(pkg, q, want, what):
    """The last warp of q against the oracle's (image, record), byte for byte."""
    want_img, want_rec = want
    got, rec = q.warped(), q.warp_record()
    assert rec.dtype == pkg.WARP_DTYPE and got.dtype == want_img.dtype and got.shape == want_img.shape, (what, got.dtype, got.shape)
    if got.tobytes() != want_img.tobytes():
        bad = np.argwhere(got != want_img)
        r, c = bad[0]
        raise AssertionError((what, "pixels differ", len(bad), (int(r), int(c)), int(got[r, c]), int(want_img[r, c])))
    assert rec.tobytes() == want_rec.tobytes(), (what, rec, want_rec)
    return got, rec


def assert_warp(pkg, q, t, h, direction, qimg, timg, fill=0, what=None, qi=0, ti=0):
    q.set_warp_model(h)
    q.warp_image(direction, qi, ti, fill)
    return assert_same(pkg, q, np_warp(h, direction, qimg, timg, fill), (what, direction))


# ---------------------------------------------------------------------------------------------
# 1. the caller's models, both directions
# ---------------------------------------------------------------------------------------------
def test_layout_and_the_state_before_any_launch(pkg):
    q, t = pair(pkg)
    with q, t:
        assert q.warp_layout() == (8, 32, 4)
        assert q.warped().shape == (0, 0) and not q.warp_record().tobytes().strip(b"\0")
        ptr, pitch, h, w, fmt, rec = q.device_warped()
        assert ptr and rec and (pitch, h, w, fmt) == (0, 0, 0, "i32")


@pytest.mark.parametrize("qfmt", ["i32", "u8"])
@pytest.mark.parametrize("tfmt", ["i32", "u8"])
def test_four_format_combinations(pkg, qfmt, tfmt):
    qimg, timg = image(QH, QW, qfmt, 1), image(TH, TW, tfmt, 2)
    q, t = pair(pkg, qfmt, tfmt)
    with q, t:
        q.set_input(qimg)
        t.set_input(timg)
        t.sync()
        covered = 0
        for direction in (0, 1):
            for name, h in (("identity", IDENTITY), ("shift", shift(5, 3)), ("back", shift(-7, -2)), ("half", shift(0.5, 0.5)),
                            ("quarter", shift(2.25, -1.75)), ("rotation", ROTATION)):
                for fill in (0, -9, 300):
                    got, rec = assert_warp(pkg, q, t, h, direction, qimg, timg, fill, (qfmt, tfmt, name, fill))
                    assert got.dtype == DT[tfmt if direction == 0 else qfmt]  # the SOURCE context's format
                    assert got.shape == ((QH, QW) if direction == 0 else (TH, TW))
                    covered += int(rec["covered"])
        assert covered > 20000  # the comparisons are not all of fill


def test_same_pattern_gives_sad_zero(pkg):
    """Query = the train image's window at (3, 8): the identity-with-shift warp reproduces it exactly."""
    timg = image(TH, TW, "i32", 3)
    qimg = np.ascontiguousarray(timg[3:3 + QH, 8:8 + QW])
    q, t = pair(pkg)
    with q, t:
        q.set_input(qimg)
        t.set_input(timg)
        t.sync()
        got, rec = assert_warp(pkg, q, t, shift(8, 3), 0, qimg, timg, -1, "window")
        assert int(rec["sad"]) == 0 and int(rec["covered"]) == QH * QW == int(rec["pixels"]) and np.array_equal(got, qimg)
        got, rec = assert_warp(pkg, q, t, shift(8, 3), 1, qimg, timg, -1, "window back")
        assert int(rec["sad"]) == 0 and int(rec["covered"]) == QH * QW and int(rec["pixels"]) == TH * TW
        assert np.array_equal(got[3:3 + QH, 8:8 + QW], qimg) and np.count_nonzero(got == -1) >= TH * TW - QH * QW
    same = image(QH, QW, "u8", 4)
    q, t = pair(pkg, "u8", "u8", tshape=(QH, QW))
    with q, t:
        q.set_input(same)
        t.set_input(same)
        t.sync()
        for direction in (0, 1):
            got, rec = assert_warp(pkg, q, t, IDENTITY, direction, same, same, 7, "identity u8")
            assert int(rec["sad"]) == 0 and int(rec["covered"]) == QH * QW and np.array_equal(got, same)


def test_edge_values_of_the_coordinates(pkg):
    qimg, timg = image(QH, QW, "i32", 5), image(TH, TW, "i32", 6)
    q, t = pair(pkg)
    with q, t:
        q.set_input(qimg)
        t.set_input(timg)
        t.sync()
        # the line w = 0 crosses the output frame: w = 20 - x
        got, rec = assert_warp(pkg, q, t, np.array([[1, 0, 0], [0, 1, 0], [-1, 0, 20]], F), 0, qimg, timg, -1, "w crosses")
        assert 0 < int(rec["covered"]) < QH * QW and np.all(got[:, 20:] == -1)
        assert_warp(pkg, q, t, np.array([[1, 0, 0], [0, 1, 0], [-1, 0, 20]], F), 1, qimg, timg, -1, "w crosses")
        # sx exactly Ws - 1 on the last column: x * (71 / 55)
        last = np.array([[71, 0, 0], [0, 55, 0], [0, 0, 55]], F)
        got, rec = assert_warp(pkg, q, t, last, 0, qimg, timg, -1, "last column")
        assert np.array_equal(got[:, QW - 1], timg[:QH, TW - 1]) and int(rec["covered"]) == QH * QW
        assert_warp(pkg, q, t, last, 1, qimg, timg, -1, "last column")
        # -0.0 coordinates: u = -0.0 * x + ... stays -0.0 on column 0 and row 0
        minus = np.array([[1, 0, -0.0], [0, 1, -0.0], [-0.0, -0.0, 1]], F)
        got, _ = assert_warp(pkg, q, t, minus, 0, qimg, timg, -1, "-0.0")
        assert np.array_equal(got, timg[:QH, :QW])
        neg = np.array([[-1, -0.0, -0.0], [-0.0, -1, -0.0], [0, 0, 1]], F)  # u = -x: -0.0 at x = 0, the only covered pixel
        got, rec = assert_warp(pkg, q, t, neg, 0, qimg, timg, -1, "-0.0 corner")
        assert int(rec["covered"]) == 1 and got[0, 0] == timg[0, 0]
        assert_warp(pkg, q, t, neg, 1, qimg, timg, -1, "-0.0 corner")
        # NaN / inf entries, one at a time and all at once; random bytes
        for k in range(9):
            for bad in (np.nan, np.inf, -np.inf):
                h = ROTATION.copy().reshape(9)
                h[k] = bad
                for direction in (0, 1):
                    assert_warp(pkg, q, t, h, direction, qimg, timg, 5, ("bad entry", k, bad))
        rng = np.random.default_rng(9)
        for i in range(8):
            h = np.frombuffer(rng.bytes(36), F)
            for direction in (0, 1):
                assert_warp(pkg, q, t, h, direction, qimg, timg, 5, ("random bytes", i))
        for direction in (0, 1):
            _, rec = assert_warp(pkg, q, t, np.full(9, np.nan, F), direction, qimg, timg, 5, "all NaN")
            assert int(rec["model"]) == 1 - direction and int(rec["covered"]) == 0
        # a singular matrix: a model in direction 0, none in direction 1
        sing = np.array([[1, 2, 3], [2, 4, 6], [0, 0, 1]], F)
        _, rec = assert_warp(pkg, q, t, sing, 0, qimg, timg, 4, "singular")
        assert int(rec["model"]) == 1
        got, rec = assert_warp(pkg, q, t, sing, 1, qimg, timg, 4, "singular")
        assert int(rec["model"]) == 0 and not rec["m"].any() and np.all(got == 4) and int(rec["covered"]) == 0
        # a mirrored model (det < 0): the sign rule
        mirror = np.array([[-0.98, 0.05, 60.0], [0.04, 0.97, 1.5], [2e-4, -1e-4, 1.0]], F)
        for direction in (0, 1):
            _, rec = assert_warp(pkg, q, t, mirror, direction, qimg, timg, -1, "mirror")
            assert int(rec["covered"]) > 1000


def test_extreme_int32_pixels(pkg):
    yy, xx = np.indices((TH, TW))
    board = np.where((yy + xx) % 2 == 0, INT32_MIN, INT32_MAX).astype(np.int32)
    qimg = image(QH, QW, "i32", 7, wide=True)
    q, t = pair(pkg)
    with q, t:
        q.set_input(qimg)
        for timg in (board, image(TH, TW, "i32", 8, wide=True)):
            t.set_input(timg)
            t.sync()
            for h in (IDENTITY, shift(0.5, 0), shift(0.5, 0.5), ROTATION):
                for direction in (0, 1):
                    _, rec = assert_warp(pkg, q, t, h, direction, qimg, timg, INT32_MIN, "extremes")
            assert int(rec["sad"]) > 2 ** 40  # a sum beyond 32 bits


def test_fill_is_clamped_for_uint8_output(pkg):
    qimg, timg = image(QH, QW, "i32", 9), image(TH, TW, "u8", 10)
    q, t = pair(pkg, "i32", "u8")
    with q, t:
        q.set_input(qimg)
        t.set_input(timg)
        t.sync()
        for fill, stored in ((-5, 0), (-2 ** 31, 0), (256, 255), (2 ** 31 - 1, 255), (200, 200)):
            got, _ = assert_warp(pkg, q, t, shift(30, 0), 0, qimg, timg, fill, ("fill", fill))
            assert got.dtype == np.uint8 and np.all(got[:, 42:] == stored)
            got, _ = assert_warp(pkg, q, t, shift(30, 0), 1, qimg, timg, fill, ("fill", fill))  # int32 output: as given
            assert got.dtype == np.int32 and np.all(got[:, :30] == fill)


# ---------------------------------------------------------------------------------------------
# 2. seams: destination sizes at the tile seams, a batch
# ---------------------------------------------------------------------------------------------
def test_destination_sizes_at_the_tile_seams(pkg):
    timg = image(TH, TW, "i32", 11)
    with pkg.PyramidContext(QH, QW, S=2, octaves=2) as probe:
        tr, tc, ppl = probe.warp_layout()
    assert tc % ppl == 0
    rows = (1, tr - 1, tr, tr + 1, 2 * tr + 1)
    cols = (1, tc - 1, tc, tc + 1, 2 * tc + 1, tc - ppl + 1)  # the last: no multiple of the pixels per lane
    sizes = {(1, 1), (1, 2 * tc + 1)} | {(r, c) for r, c in zip(rows, cols)} | {(r, c) for r, c in zip(rows[::-1], cols)}
    sizes |= {(2 * tr + 1, tc - ppl + 1), (tr, 2 * tc + 1), (4 * tr + 1, 4 * tc + 2)}  # the last: more than one block both ways
    for fmt in ("i32", "u8"):
        for hd, wd in sorted(sizes) if fmt == "i32" else ((1, 1), (tr + 1, tc - ppl + 1), (2 * tr + 1, 2 * tc + 1)):
            qimg = image(hd, wd, fmt, 12)
            q, t = pair(pkg, fmt, "i32", qshape=(hd, wd))
            with q, t:
                q.set_input(qimg)
                t.set_input(timg)
                t.sync()
                for h in (shift(0.5, 0.25), ROTATION):
                    got, rec = assert_warp(pkg, q, t, h, 0, qimg, timg, -3, ("seam", fmt, hd, wd))
                    assert got.shape == (hd, wd) and int(rec["pixels"]) == hd * wd
                    assert_warp(pkg, q, t, h, 1, qimg, timg, -3, ("seam back", fmt, hd, wd))  # the source is hd x wd


def test_batch_three_picks_its_images(pkg):
    qimgs = [image(QH, QW, "i32", 20 + b) for b in range(3)]
    timgs = [image(TH, TW, "i32", 30 + b) for b in range(3)]
    q, t = pair(pkg, batch=3)
    with q, t:
        for b in range(3):
            q.set_input(qimgs[b], b)
            t.set_input(timgs[b], b)
        t.sync()
        for direction in (0, 1):
            q.set_warp_model(ROTATION)
            q.warp_image(direction, 2, 1, -1)
            assert_same(pkg, q, np_warp(ROTATION, direction, qimgs[2], timgs[1], -1), ("batch", direction))


# ---------------------------------------------------------------------------------------------
# 3. the pipeline on one stream: build ... match, fit, warp, with no host read in between
# ---------------------------------------------------------------------------------------------
def scene(oracle):
    """A train image and the query image that is its window at (4, 8): the model is a translation."""
    timg = oracle.lcg_image(TH, TW, 4321)
    return np.ascontiguousarray(timg[4:4 + QH, 8:8 + QW]), timg


def run_chain(q, t, qimg, timg):
    for ctx, img in ((q, qimg), (t, timg)):
        ctx.set_input(img)
        ctx.build_gaussian()
        ctx.detect_extrema()
        ctx.refine_keypoints(0.5, 10.0)
        ctx.orient_keypoints()
        ctx.describe_keypoints()
    t.sync()  # the train context's own stream: the one ordering the caller owes


def test_pipeline_on_one_stream(pkg, oracle):
    qimg, timg = scene(oracle)
    with pkg.PyramidContext(QH, QW, S=2, octaves=2) as q, pkg.PyramidContext(TH, TW, S=2, octaves=2) as t:
        run_chain(q, t, qimg, timg)
        for direction in (0, 1):
            q.match_descriptors(t, ratio=0.0)
            q.fit_homography(512, 3, 2.0)
            q.warp_image(direction, fill=-1)  # the same stream, no synchronisation and no host read above
            model = q.homography()
            M = raw_matches(pkg, q)
            assert len(M) >= 4 and model.matrix is not None, (len(M), model)  # the test cannot pass empty
            got, rec = assert_same(pkg, q, np_warp_model(model, direction, qimg, timg, -1), ("pipeline", direction))
            print(f"direction {direction}: {len(M)} matches, {int(model['inliers'])} inliers, covered {int(rec['covered'])}, "
                  f"sad {int(rec['sad'])}")
            assert int(rec["covered"]) > QH * QW // 2
        # the "none" model: min_inliers above the list length
        q.fit_homography(64, 3, 2.0, min_inliers=len(M) + 1)
        for direction in (0, 1):
            q.warp_image(direction, fill=77)
            model = q.homography()
            assert int(model["hypothesis"]) == NONE
            got, rec = assert_same(pkg, q, np_warp_model(model, direction, qimg, timg, 77), ("none", direction))
            assert np.all(got == 77) and int(rec["covered"]) == 0 and int(rec["model"]) == 0 and int(rec["sad"]) == 0
        # a caller's model, then back to the fit's record
        assert_warp(pkg, q, t, ROTATION, 0, qimg, timg, 1, "own")
        q.set_warp_model(None)
        q.warp_image(0, fill=77)
        assert np.all(q.warped() == 77) and int(q.warp_record()["model"]) == 0


# ---------------------------------------------------------------------------------------------
# 4. state: the warp only reads
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
        for direction in (0, 1):
            q.warp_image(direction, fill=-1)
            assert_same(pkg, q, np_warp_model(q.homography(), direction, qimg, timg, -1), ("state", direction))
            assert state() == before
        assert_warp(pkg, q, t, ROTATION, 1, qimg, timg, 3, "state, own model")
        assert state() == before
        for ctx in (q, t):  # the next build is still the steady-state one
            ctx.build()
            assert ctx.tuning()["zeros_clean"] == 1
        assert (q.checksum(0), t.checksum(0)) == (before[0][0], before[1][0])


# ---------------------------------------------------------------------------------------------
# 5. consumers: a third context binds the output; a bound source buffer
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("qfmt,tfmt,direction", [("i32", "i32", 0), ("u8", "u8", 0), ("i32", "u8", 1), ("u8", "i32", 1), ("i32", "u8", 0)])
def test_a_third_context_builds_on_the_warped_image(pkg, oracle, qfmt, tfmt, direction):
    qimg, timg = image(QH, QW, qfmt, 40), image(TH, TW, tfmt, 41)
    q, t = pair(pkg, qfmt, tfmt)
    with q, t:
        q.set_input(qimg)
        t.set_input(timg)
        t.sync()
        want, _ = assert_warp(pkg, q, t, ROTATION, direction, qimg, timg, 3, "consumer")
        ptr, pitch, h, w, fmt, _ = q.device_warped()
        assert (h, w) == want.shape and fmt == (tfmt if direction == 0 else qfmt) and pitch % 4 == 0 and w <= pitch < w + 4
        with pkg.PyramidContext(h, w, S=2, input_format=fmt) as c:
            c.bind_device_input(ptr, pitch, pitch * h)
            c.build(q.stream)  # behind the warp, on its stream
            q.sync()
            got = c.pyramid(0)
            ref = oracle.build_pyramid(want.astype(np.int32), 2)
            assert got.shape == ref.shape and np.array_equal(got.view(np.uint32), ref.view(np.uint32))
            c.unbind_device_input()


@pytest.mark.parametrize("fmt,pitch", [("i32", 75), ("i32", 76), ("u8", 75), ("u8", 128)])
def test_a_bound_pitched_source_gives_the_same_output(pkg, fmt, pitch):
    import torch

    qimg, timg = image(QH, QW, fmt, 50), image(TH, TW, fmt, 51)
    q, t = pair(pkg, fmt, fmt)
    with q, t:
        q.set_input(qimg)
        t.set_input(timg)
        t.sync()
        own, _ = assert_warp(pkg, q, t, ROTATION, 0, qimg, timg, 3, "own buffer")
        back, _ = assert_warp(pkg, q, t, ROTATION, 1, qimg, timg, 3, "own buffer")  # the train image as the frame
        host = np.full((TH, pitch), 99, DT[fmt])
        host[:, :TW] = timg
        dev = torch.from_numpy(host).cuda()
        torch.cuda.synchronize()
        t.bind_device_input(dev.data_ptr(), pitch, TH * pitch, keepalive=dev)
        bound, _ = assert_warp(pkg, q, t, ROTATION, 0, qimg, timg, 3, ("bound source", pitch))
        assert bound.tobytes() == own.tobytes()
        bound, _ = assert_warp(pkg, q, t, ROTATION, 1, qimg, timg, 3, ("bound frame", pitch))
        assert bound.tobytes() == back.tobytes()
        t.unbind_device_input()


# ---------------------------------------------------------------------------------------------
# 6. refusals
# ---------------------------------------------------------------------------------------------
def test_refusals_leave_the_previous_result(pkg):
    L = pkg.lib()
    qimg, timg = image(QH, QW, "i32", 60), image(TH, TW, "i32", 61)
    q, t = pair(pkg)
    with q, t:
        q.set_input(qimg)
        t.set_input(timg)
        t.sync()
        want = np_warp(ROTATION, 0, qimg, timg, 2)
        assert_warp(pkg, q, t, ROTATION, 0, qimg, timg, 2, "before")
        for args, word in (((2, 0, 0), "direction"), ((-1, 0, 0), "direction"), ((0, 1, 0), "out of range"), ((0, -1, 0), "out of range"),
                           ((1, 0, 1), "out of range"), ((1, 0, -1), "out of range")):
            with pytest.raises(pkg.GdpError) as e:
                q.warp_image(*args, fill=9)
            assert e.value.status == 1 and word in str(e.value), (args, str(e.value))
            assert_same(pkg, q, want, ("after a refusal", args))
        w = q._warp_handle()
        host = np.zeros((QH, QW), np.int32)
        assert L.gdp_download_warped(w, ctypes.c_void_p(host.ctypes.data), QW - 1) == 1 and not host.any()
        assert b"pitch" in L.gdp_warp_last_error(w)
        assert L.gdp_download_warped(w, None, QW) == 1
        wide = np.full((QH, QW + 5), -8, np.int32)
        assert L.gdp_download_warped(w, ctypes.c_void_p(wide.ctypes.data), QW + 5) == 0
        assert np.array_equal(wide[:, :QW], want[0]) and np.all(wide[:, QW:] == -8)
        assert L.gdp_download_warp_record(w, None) == 1
        with pytest.raises(ValueError):
            q.set_warp_model(np.zeros(8, F))


def test_a_row_band_is_refused(pkg):
    with pkg.PyramidContext(64, 64, S=2, octaves=2, row_begin=0, row_end=32) as band:
        with pytest.raises(pkg.GdpError) as e:
            band.warp_image()
        assert e.value.status == 3 and "row band" in str(e.value)  # GDP_ERR_STATE


# ---------------------------------------------------------------------------------------------
# 7. the C++ example, executed
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("direction", [0, 1])
def test_cpp_example_gives_the_python_paths_record(pkg, oracle, direction):
    """Two 64 x 64 LCG images, the second moved 16 columns to the right.  The example fits the matches
    sorted by their coordinates and warps under the fitted matrix: its record's bits and its image's
    checksum must be those of the Python path on the same sorted list."""
    exe = os.path.join(REPO, "examples", "warp_hip")
    if not os.path.exists(exe):
        subprocess.run(["make", "-s", "-C", os.path.join(REPO, "examples"), "warp_hip"], check=True)
    n, S, seed, move = 64, 2, 12345, 16
    out = subprocess.run([exe, str(n), str(S), f"lcg:{seed}", str(move), "0.5", "10", "0.8", "256", "7", "3.0", str(direction), "-1"],
                         check=True, timeout=120, capture_output=True, text=True).stdout
    print(out)
    head = re.search(r"^warped (\d+) x (\d+) checksum (\d+)\nmodel (\d+) covered (\d+) pixels (\d+) sad (\d+) direction (\d+) reserved (\d+)\n",
                     out, re.M)
    assert head, out
    hbits = [int(word, 16) for row in re.findall(r"^h (\w{8}) (\w{8}) (\w{8})", out, re.M) for word in row]
    mbits = [int(word, 16) for row in re.findall(r"^m (\w{8}) (\w{8}) (\w{8})", out, re.M) for word in row]
    img = oracle.lcg_image(n, n, seed)
    moved = np.ascontiguousarray(np.roll(img, move, axis=1))
    with pkg.PyramidContext(n, n, S=S) as a, pkg.PyramidContext(n, n, S=S) as b:
        run_chain(a, b, img, moved)
        a.match_descriptors(b, ratio=0.8, mutual=True)
        M = np.asarray(a.matches())
        M = M[np.lexsort((M["second"], M["distance"], M["ty"], M["tx"], M["qy"], M["qx"]))]
        a.set_ransac_input(M)
        a.fit_homography(256, 7, 3.0)
        model = a.homography()
        assert hbits == [int(w) for w in model["h"].view(np.uint32)]
        a.set_warp_model(model["h"])
        a.warp_image(direction, fill=-1)
        got, rec = assert_same(pkg, a, np_warp(model["h"], direction, img, moved, -1), ("example", direction))
    assert model.matrix is not None and int(rec["covered"]) > n * n // 2
    flat = got.reshape(-1).astype(np.int64) & 0xFFFFFFFF
    checksum = int((flat.astype(object) * (np.arange(flat.size) % 65521 + 1).astype(object)).sum()) & (2 ** 64 - 1)
    want = [n, n, checksum, int(rec["model"]), int(rec["covered"]), int(rec["pixels"]), int(rec["sad"]), direction, 0]
    assert [int(x) for x in head.groups()] == want
    assert mbits == [int(w) for w in rec["m"].view(np.uint32)]
    assert WARP_DT.itemsize == 64
