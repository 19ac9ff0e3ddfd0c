"""On-device scale-space extrema (gdp_detect_extrema) against a numpy float32 oracle that implements
the rules of include/gdp.h literally.  The result is a set and is compared exactly: position, kind
and the bits of the value.  Most cases run on UPLOADED pyramids, independent of any build kernel."""
import numpy as np
import pytest

from extrema_oracle import (BIG, ODD, F, as_set, assert_short_downloads, assert_sorted, small_pipeline, detect, normal_pyramid, np_extrema, octave_levels,
                            packed_size, smooth_pyramid, tie_pyramid, want)

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------
# uploaded pyramids
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [BIG, ODD], ids=["200x520", "37x100"])
def test_normal_levels_exact_set(pkg, shape):
    H, W, S, O = shape
    expect, _ = want("normal", shape)
    assert len(expect) > 500
    kp = detect(pkg, normal_pyramid(shape), H, W, S, octaves=0)
    assert kp.found == len(kp) == len(expect)
    assert as_set(kp) == expect
    assert {k[0] for k in expect} >= {0, 1, 2}  # several octaves, the odd-width ones included


def test_ties_and_special_values_exact_set(pkg):
    H, W, S, O = BIG
    p = tie_pyramid(BIG)
    expect, _ = want("tie", BIG)
    assert 100 < len(expect) < 20000  # strictness: far fewer than the ~7 % of iid levels
    assert np.isnan(p).any() and np.isinf(p).any() and (np.abs(p[p != 0]) < 1e-38).any()
    kp = detect(pkg, p, H, W, S)
    assert as_set(kp) == expect
    assert {k[2] for k in expect} == {1, -1}


@pytest.mark.parametrize("S,shape", [(4, (20, 40)), (5, (24, 36)), (7, (12, 20))])
def test_more_than_three_candidate_levels(pkg, S, shape):
    """S > 3 is detected in chunks of three candidate levels (the last chunk overlaps the one
    before it): every level is reported exactly once."""
    H, W = shape
    O = 2
    p = np.random.default_rng(S).standard_normal(packed_size(H, W, S, O), dtype=np.float32)
    expect, _ = np_extrema(p, H, W, S, O)
    assert {k[1] for k in expect} == set(range(1, S + 1))
    kp = detect(pkg, p, H, W, S, octaves=O)
    assert as_set(kp) == expect


# ---------------------------------------------------------------------------------------------
# contrast and edge rejection
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("contrast", [0.5, 2.0])
def test_contrast_threshold(pkg, contrast):
    H, W, S, O = BIG
    expect, _ = want("normal", BIG, contrast=contrast)
    everything, _ = want("normal", BIG)
    assert 0 < len(expect) < len(everything)
    assert as_set(detect(pkg, normal_pyramid(BIG), H, W, S, contrast=contrast)) == expect


@pytest.mark.parametrize("kind,contrast,edge_ratio", [("normal", 0.0, 1.5), ("normal", 0.5, 1.5), ("smooth", 0.0, 3.0)])
def test_edge_rejection(pkg, kind, contrast, edge_ratio):
    H, W, S, O = BIG
    expect, before = want(kind, BIG, contrast=contrast, edge_ratio=edge_ratio)
    rejected = 1.0 - len(expect) / before
    print(f"edge test rejects {rejected:.3f} of {before} contrast-passing extrema")
    assert 0.10 < rejected < 0.90  # the check cannot pass vacuously
    src = {"normal": normal_pyramid, "smooth": smooth_pyramid}[kind](BIG)
    assert as_set(detect(pkg, src, H, W, S, contrast=contrast, edge_ratio=edge_ratio)) == expect


def test_invalid_arguments(pkg):
    with pkg.PyramidContext(64, 64, S=2) as ctx:
        for contrast, edge_ratio in [(-1.0, 0.0), (float("nan"), 0.0), (0.0, 0.5), (0.0, float("inf")),
                                     (0.0, float("nan")), (0.0, -2.0)]:
            with pytest.raises(pkg.GdpError) as e:
                ctx.detect_extrema(contrast, edge_ratio)
            assert e.value.status == 1, (contrast, edge_ratio)
        with pytest.raises(pkg.GdpError) as e:
            ctx.set_keypoint_capacity(0)
        assert e.value.status == 1


# ---------------------------------------------------------------------------------------------
# degenerate geometry
# ---------------------------------------------------------------------------------------------
def test_no_scales_gives_nothing(pkg):
    p = np.random.default_rng(1).standard_normal(packed_size(64, 64, 0, 7), dtype=np.float32)
    kp = detect(pkg, p, 64, 64, 0)
    assert len(kp) == 0 and kp.found == 0 and kp.dtype == pkg.KEYPOINT_DTYPE


def test_batch_images_are_independent(pkg):
    H, W, S, B = 48, 272, 1, 3
    O = 6
    rng = np.random.default_rng(7)
    imgs = [rng.standard_normal(packed_size(H, W, S, O), dtype=np.float32) for _ in range(B)]
    with pkg.PyramidContext(H, W, S=S, batch=B) as ctx:
        assert ctx.O == O
        for b, p in enumerate(imgs):
            ctx.upload_pyramid(p, b)
        ctx.detect_extrema()
        sets = []
        for b, p in enumerate(imgs):
            expect, _ = np_extrema(p, H, W, S, O)
            assert len(expect) > 300
            kp = ctx.keypoints(b)
            assert_sorted(kp)
            assert as_set(kp) == expect, b
            sets.append(expect)
        assert sets[0] != sets[1] != sets[2]


def test_three_by_three_octave_has_one_candidate(pkg):
    H, W, S, O = 12, 12, 2, 3
    p = np.random.default_rng(3).standard_normal(packed_size(H, W, S, O), dtype=np.float32)
    octave_levels(p, H, W, S, O)[2][1, 1, 1] = F(100)  # the only candidate of level (2, 1): a maximum
    octave_levels(p, H, W, S, O)[2][2] = F(-100)       # level (2, 2): its candidate ties with its neighbours
    expect, _ = np_extrema(p, H, W, S, O)
    assert [k for k in expect if k[0] == 2] == [(2, 1, 1, 1, 1, int(F(100).view(np.uint32)))]
    assert as_set(detect(pkg, p, H, W, S, octaves=O)) == expect


# ---------------------------------------------------------------------------------------------
# capacity overflow
# ---------------------------------------------------------------------------------------------
def test_capacity_overflow_keeps_the_count_and_the_bounds(pkg):
    """found counts every keypoint, exactly `capacity` distinct true ones are stored, and image 0's
    overflow writes nothing into image 1's records, which follow its own in the buffer."""
    H, W, S, B, cap = 48, 272, 1, 2, 100
    O = 6
    rng = np.random.default_rng(11)
    imgs = [rng.standard_normal(packed_size(H, W, S, O), dtype=np.float32) for _ in range(B)]
    expects = [np_extrema(p, H, W, S, O)[0] for p in imgs]
    assert all(len(e) > 10 * cap for e in expects) and not (expects[0] & expects[1])
    with pkg.PyramidContext(H, W, S=S, batch=B) as ctx:
        ctx.set_keypoint_capacity(cap)
        for b, p in enumerate(imgs):
            ctx.upload_pyramid(p, b)
        ctx.detect_extrema()
        recs = [ctx.device_keypoints(b)[0] for b in range(B)]
        assert recs[1] - recs[0] == cap * 16
        for b in range(B):
            kp = ctx.keypoints(b)
            assert kp.found == ctx.keypoint_count(b) == len(expects[b])
            assert len(kp) == cap
            assert as_set(kp) <= expects[b], b
            assert_sorted(kp)
        ctx.set_keypoint_capacity(65536)  # ample: the set is complete
        ctx.detect_extrema()
        for b in range(B):
            assert as_set(ctx.keypoints(b)) == expects[b], b


def test_detection_is_reproducible(pkg):
    H, W, S, O = ODD
    with pkg.PyramidContext(H, W, S=S) as ctx:
        ctx.upload_pyramid(normal_pyramid(ODD))
        ctx.detect_extrema(0.25, 5.0)
        first = ctx.keypoints(0)
        ctx.detect_extrema(0.25, 5.0)
        second = ctx.keypoints(0)
    assert len(first) > 50 and first.tobytes() == second.tobytes()


# ---------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------
def test_after_build_gaussian(pkg, oracle):
    H, W, S = 96, 520, 2
    with pkg.PyramidContext(H, W, S=S) as ctx:
        ctx.set_input(oracle.lcg_image(H, W, 12345))
        ctx.build_gaussian()
        ctx.detect_extrema()
        kp = ctx.keypoints(0)
        expect, _ = np_extrema(ctx.pyramid(0), H, W, S, ctx.O)
    assert len(expect) > 100 and as_set(kp) == expect


def test_after_window_build(pkg, oracle):
    """The reference's window pyramid: few keypoints, and its +0 plateaus give none."""
    n, S = 64, 2
    with pkg.PyramidContext(n, n, S=S) as ctx:
        ctx.set_input(oracle.lcg_image(n, n, 12345))
        ctx.build()
        ctx.detect_extrema()
        kp = ctx.keypoints(0)
        packed = ctx.pyramid(0)
        expect, _ = np_extrema(packed, n, n, S, ctx.O)
    assert as_set(kp) == expect
    assert all(k[5] & 0x7FFFFFFF for k in expect)  # no zero-valued keypoint


@pytest.mark.parametrize("defer", [False, True])
def test_dropin_class_detects_on_host_edits(pkg, oracle, defer):
    n, S = 64, 2
    g = pkg.GaussPyramid(oracle.lcg_image(n, n, 7), n, S, defer=defer)
    try:
        g.GenerateDoG()
        kp = g.DetectExtrema()
        expect, _ = np_extrema(g.pyramid(), n, n, S, g.layer)
        assert as_set(kp) == expect
        planted = (0, 1, 1, 5, 5, int(F(1e6).view(np.uint32)))
        assert planted not in expect
        g.GaussPy[0][1][5][5] = 1e6
        kp = g.DetectExtrema()
        assert planted in as_set(kp)
        expect, _ = np_extrema(g.pyramid(), n, n, S, g.layer)  # the device pyramid now holds the edit
        assert planted in expect and as_set(kp) == expect
        assert g.GaussPy[0][1][5][5] == F(1e6) and g.GaussPy[0][1][5][6] != F(1e6)  # GaussPy left alone
    finally:
        g.close()


# ---------------------------------------------------------------------------------------------
# refusals and placement
# ---------------------------------------------------------------------------------------------
def test_band_context_is_refused(pkg):
    with pkg.PyramidContext(64, 64, S=2, octaves=5, row_begin=0, row_end=32) as ctx:
        with pytest.raises(pkg.GdpError) as e:
            ctx.detect_extrema()
        assert e.value.status == 3 and "band" in str(e.value)


def test_on_a_caller_stream(pkg, oracle):
    import torch

    H, W, S = 96, 520, 2
    stream = torch.cuda.Stream()
    assert stream.cuda_stream != 0
    with pkg.PyramidContext(H, W, S=S) as ctx:
        ctx.set_input(oracle.lcg_image(H, W, 99), stream=stream)
        ctx.build_gaussian(stream)
        ctx.detect_extrema(0.0, 10.0, stream=stream)
        stream.synchronize()
        kp = ctx.keypoints(0)
        expect, _ = np_extrema(ctx.pyramid(0), H, W, S, ctx.O, edge_ratio=10.0)
    assert len(expect) > 50 and as_set(kp) == expect


def test_on_a_bound_output_buffer(pkg):
    import torch

    H, W, S, O = ODD
    expect, _ = want("normal", ODD)
    with pkg.PyramidContext(H, W, S=S) as ctx:
        buf = torch.full((ctx.pyramid_bytes() // 4,), float("nan"), device="cuda")
        ctx.bind_device_output(buf.data_ptr(), ctx.pyramid_bytes(), keepalive=buf)
        ctx.upload_pyramid(normal_pyramid(ODD))  # lands in the bound buffer
        ctx.detect_extrema(stream=torch.cuda.current_stream())
        torch.cuda.current_stream().synchronize()
        assert as_set(ctx.keypoints(0)) == expect
        off = ctx.level_offset(0, 0, 1)
        assert torch.equal(buf[off:off + 4].cpu(), torch.from_numpy(octave_levels(normal_pyramid(ODD), H, W, S, O)[0][1, 0, :4].copy()))
        ctx.unbind_device_output()


def test_download_through_a_short_buffer_and_through_none(pkg, oracle):
    L = pkg.lib()
    with small_pipeline(pkg, oracle, 1) as ctx:
        assert_short_downloads(lambda *a: L.gdp_download_keypoints(ctx._ctx, 0, *a), ctx.keypoints(0))
