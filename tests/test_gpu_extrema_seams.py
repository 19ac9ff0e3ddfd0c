"""k_extrema pinned at its seams, all comparisons exact sets (octave, scale, kind, row, col, value
bits): the strip seam (a wave owns 62 groups = 248 columns, lanes 0 / 63 are halo lanes), the tile
seam (16 candidate rows, a two-row loop with a row look-ahead), both load paths (cols % 4), every
k_extrema<1|2|3> and the chunked S > 3, the values where a comparison can go wrong (one ulp, ties,
denormals, one-signed data, |v| == contrast, NaN / inf in the edge test), the work-unit decode with
batch x chunks x octaves x tiles x strips, the capacity boundary, the zero-copy view and the C++
drop-in.  The lattice pyramids' keypoints are known in closed form (tests/extrema_oracle.py)."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

from extrema_oracle import (BIG, PHASES, F, as_set, assert_sorted, denormal_pyramid, detect, lattice_pyramid, np_extrema,
                            one_signed_pyramid, packed_size, tie_pyramid, want)

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(x):
    return int(F(x).view(np.uint32))


def magnitude(k):
    return k[5] & 0x7FFFFFFF


# ---------------------------------------------------------------------------------------------
# one neighbour decides: the lattice pyramids
# ---------------------------------------------------------------------------------------------
def run_lattice(pkg, H, W, S, O, batch):
    """Every phase and both signs; image b of a launch carries rotation first + b.  Returns the
    number of keypoints seen."""
    assert 27 % batch == 0
    seen = 0
    with pkg.PyramidContext(H, W, S=S, octaves=O, batch=batch) as ctx:
        assert ctx.O == O
        for n, phase in enumerate(PHASES):
            for sigma in (1, -1):
                for first in range(0, 27, batch):
                    expects, kept = [], None
                    for b in range(batch):
                        p, e = lattice_pyramid(H, W, S, O, phase, first + b, sigma)
                        ctx.upload_pyramid(p, b)
                        expects.append(e)
                        if first + b == n:  # the image that is also judged by the oracle: another one per phase
                            kept = (b, p)
                    ctx.detect_extrema()
                    for b in range(batch):
                        kp = ctx.keypoints(b)
                        assert kp.found == len(kp)
                        assert as_set(kp) == expects[b], (phase, sigma, first + b)
                        seen += len(kp)
                    if kept:
                        b, p = kept
                        kp = ctx.keypoints(b)
                        assert_sorted(kp)
                        assert as_set(kp) == np_extrema(p, H, W, S, O)[0], (phase, sigma, first + b)
    return seen


def candidates(H, W, S, O):
    return sum(S * ((H >> o) - 2) * ((W >> o) - 2) for o in range(O) if (H >> o) >= 3 and (W >> o) >= 3)


LATTICE_SHAPES = [
    (3, 3, 1),      # smallest octave with a candidate
    (4, 4, 2),      # smallest vector-path octave
    (17, 5, 3),     # 15 candidate rows
    (18, 8, 4),     # 16 candidate rows, chunked S
    (19, 247, 2),   # one strip, scalar path
    (20, 248, 3),   # exactly one full strip, vector path
    (34, 249, 1),   # second strip holds only column cols-1
    (35, 250, 5),   # second strip with one candidate column
    (19, 251, 7),   # second strip, scalar path, chunked S
    (20, 252, 2),   # second strip, vector path
    (34, 253, 3),   # second strip, scalar path
    (18, 256, 4),   # second strip, vector path, chunked S
    (35, 496, 2),   # exactly two full strips
    (36, 497, 3),   # third strip
    (19, 500, 1),   # third strip
    (35, 501, 2),   # third strip, scalar path
]


@pytest.mark.parametrize("shape", LATTICE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_lattice_one_neighbour_decides(pkg, shape):
    """27 images per launch (rotation = image index), 54 launches: every candidate is a keypoint
    once per sign, and each of its 26 neighbours blocks it once, by a tie one ulp above the rest."""
    rows, cols, S = shape
    assert run_lattice(pkg, rows, cols, S, 1, batch=27) == 2 * candidates(rows, cols, S, 1)


def test_lattice_on_three_octaves(pkg):
    """Octaves 70 x 1000, 35 x 500 and 17 x 250 (27 images per launch): the octave decode of a work
    unit with several strips and tiles in the later octaves."""
    H, W, S, O = 70, 1000, 2, 3
    assert run_lattice(pkg, H, W, S, O, batch=27) == 2 * candidates(H, W, S, O)


# ---------------------------------------------------------------------------------------------
# value edges on random pyramids whose octaves cross the seams on both load paths
# ---------------------------------------------------------------------------------------------
SEAM_A = (140, 1002, 2, 8)  # widths 1002 / 501 / 250 / 125 / 62 / 31 / 15 / 7
SEAM_B = (140, 1000, 3, 8)  # widths 1000 / 500 / 250 / 125 / ...
SEAMS = pytest.mark.parametrize("shape", [SEAM_A, SEAM_B], ids=["140x1002", "140x1000"])


@functools.lru_cache(maxsize=None)
def expected(make, shape, arg, contrast=0.0):
    return np_extrema(make(shape, arg), *shape, contrast=contrast)[0]


@SEAMS
@pytest.mark.parametrize("sign", [1, -1])
def test_one_signed_values(pkg, shape, sign):
    """All values in [1, 2) (or (-2, -1]): a 0 from a lane without a shift source, or a pixel
    clamped into the row, taken as a neighbour, blocks minima (maxima) or lets others through."""
    H, W, S, O = shape
    expect = expected(one_signed_pyramid, shape, sign)
    assert len(expect) > 500 and {k[2] for k in expect} == {1, -1}
    assert as_set(detect(pkg, one_signed_pyramid(shape, sign), H, W, S)) == expect


@SEAMS
def test_distinct_denormals(pkg, shape):
    """Every value a denormal: as centre, as neighbour and against a denormal contrast threshold
    that equals the |value| of one keypoint (which it therefore removes)."""
    H, W, S, O = shape
    p = denormal_pyramid(shape, 2 ** 20)
    expect = expected(denormal_pyramid, shape, 2 ** 20)
    assert len(expect) > 500 and all(0 < magnitude(k) < 0x00800000 for k in expect)  # biased exponent 0
    assert as_set(detect(pkg, p, H, W, S)) == expect
    thr = np.uint32(sorted(magnitude(k) for k in expect)[len(expect) // 2]).view(np.float32)
    assert 0 < thr < F(1.2e-38)
    strong = expected(denormal_pyramid, shape, 2 ** 20, contrast=float(thr))
    assert 0.1 * len(expect) < len(expect) - len(strong) < 0.9 * len(expect)
    assert strong < expect and any(magnitude(k) == bits(thr) for k in expect - strong)
    assert as_set(detect(pkg, p, H, W, S, contrast=float(thr))) == strong


@SEAMS
def test_denormal_ties(pkg, shape):
    H, W, S, O = shape
    expect = expected(denormal_pyramid, shape, 3)
    assert 0 < len(expect) < 5000 and all(magnitude(k) in (1, 2, 3) for k in expect)
    assert as_set(detect(pkg, denormal_pyramid(shape, 3), H, W, S)) == expect


def test_contrast_is_strictly_greater(pkg):
    """tie_pyramid holds |v| == 2 and |v| == 3 keypoints: contrast 2 removes the former, contrast 3
    everything finite (a kernel comparing with >= keeps them)."""
    H, W, S, O = BIG
    everything, _ = want("tie", BIG)
    for contrast, left in ((2.0, (bits(3), bits(np.inf))), (3.0, (bits(np.inf),))):
        expect, _ = want("tie", BIG, contrast=contrast)
        assert expect and {magnitude(k) for k in expect} == set(left)
        assert len([k for k in everything - expect if magnitude(k) == bits(contrast)]) >= 5
        assert as_set(detect(pkg, tie_pyramid(BIG), H, W, S, contrast=contrast)) == expect


@pytest.mark.parametrize("edge_ratio", [1.5, 10.0])
def test_edge_test_on_ties_and_special_values(pkg, edge_ratio):
    """The edge test where its arithmetic meets ties (det == 0), NaN and inf: every +-inf keypoint
    is rejected through inf - inf = NaN."""
    H, W, S, O = BIG
    everything, _ = want("tie", BIG)
    expect, before = want("tie", BIG, edge_ratio=edge_ratio)
    assert before == len(everything) and 0 < len(expect) < before
    assert any(magnitude(k) == bits(np.inf) for k in everything)
    assert not any(magnitude(k) == bits(np.inf) for k in expect)
    assert as_set(detect(pkg, tie_pyramid(BIG), H, W, S, edge_ratio=edge_ratio)) == expect


# ---------------------------------------------------------------------------------------------
# decode, capacity and zero-copy: a batch of three images with chunked levels
# ---------------------------------------------------------------------------------------------
CHUNKED = (40, 520, 2)  # octaves 40 x 520 (3 tiles x 3 strips) and 20 x 260 (2 x 2)
CHUNKED_S = pytest.mark.parametrize("S", [4, 7])


@functools.lru_cache(maxsize=None)
def chunked_batch(S):
    H, W, O = CHUNKED
    rng = np.random.default_rng(100 + S)
    imgs = [rng.standard_normal(packed_size(H, W, S, O), dtype=np.float32) for _ in range(3)]
    expects = [np_extrema(p, H, W, S, O)[0] for p in imgs]
    for e in expects:
        assert {(k[0], k[1]) for k in e} == {(o, s) for o in range(O) for s in range(1, S + 1)}
    assert not (expects[0] & expects[1]) and not (expects[1] & expects[2]) and not (expects[0] & expects[2])
    return imgs, expects


def device_records(pkg, ctx, b, capacity):
    """(records, counter) of image b copied from the addresses gdp_device_keypoints returns."""
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    ctx.keypoint_count(b)  # blocking: the detection has finished
    recs_ptr, count_ptr = ctx.device_keypoints(b)
    recs = np.zeros(capacity, pkg.KEYPOINT_DTYPE)
    count = np.zeros(1, np.uint32)
    assert hip.hipMemcpy(recs.ctypes.data, recs_ptr, recs.nbytes, 2) == 0  # hipMemcpyDeviceToHost (synchronous)
    assert hip.hipMemcpy(count.ctypes.data, count_ptr, count.nbytes, 2) == 0
    return recs, int(count[0])


@CHUNKED_S
def test_batch_of_chunked_levels(pkg, S):
    """batch 3 x level chunks x 2 octaves x tiles x strips: every image's set is exact, and the
    device records and counter read through device_keypoints are the same set."""
    H, W, O = CHUNKED
    imgs, expects = chunked_batch(S)
    capacity = 16384
    assert all(len(e) < capacity for e in expects)
    with pkg.PyramidContext(H, W, S=S, octaves=O, batch=3) as ctx:
        ctx.set_keypoint_capacity(capacity)
        for b, p in enumerate(imgs):
            ctx.upload_pyramid(p, b)
        ctx.detect_extrema()
        for b in range(3):
            kp = ctx.keypoints(b)
            assert_sorted(kp)
            assert kp.found == ctx.keypoint_count(b) == len(expects[b])
            assert as_set(kp) == expects[b], b
            recs, count = device_records(pkg, ctx, b, capacity)
            assert count == len(expects[b])
            assert as_set(recs[:count]) == expects[b], b


@CHUNKED_S
@pytest.mark.parametrize("delta", [0, -1, 1])
def test_capacity_at_the_boundary(pkg, S, delta):
    """capacity == found, found - 1 and found + 1 of image 0: the count is unchanged, min(found,
    capacity) distinct true keypoints are stored, and nothing spills into image 1's records, which
    follow image 0's in the buffer."""
    H, W, O = CHUNKED
    imgs, expects = chunked_batch(S)
    capacity = len(expects[0]) + delta
    with pkg.PyramidContext(H, W, S=S, octaves=O, batch=3) as ctx:
        ctx.set_keypoint_capacity(capacity)
        for b, p in enumerate(imgs):
            ctx.upload_pyramid(p, b)
        ctx.detect_extrema()
        assert ctx.device_keypoints(1)[0] - ctx.device_keypoints(0)[0] == capacity * 16
        for b in range(3):
            found = len(expects[b])
            kp = ctx.keypoints(b)
            assert_sorted(kp)
            assert kp.found == ctx.keypoint_count(b) == found
            assert len(kp) == min(found, capacity)
            got = as_set(kp)
            assert got <= expects[b], b
            if found <= capacity:
                assert got == expects[b], b
            recs, count = device_records(pkg, ctx, b, capacity)
            assert count == found
            assert as_set(recs[:min(count, capacity)]) == got, b


# ---------------------------------------------------------------------------------------------
# the C++ drop-in class, executed
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("edge_ratio", [0.0, 10.0])
@pytest.mark.parametrize("n", [64, 100])
def test_cpp_dropin_detect_extrema(pkg, tmp_path, n, edge_ratio):
    """examples/extrema_hip: GaussPyramid_hip(n, S), GenerateDoG(), DetectExtrema() through plain
    g++; its records are sorted and are the oracle's set on the pyramid it wrote."""
    exe = os.path.join(REPO, "examples", "extrema_hip")
    if not os.path.exists(exe):
        subprocess.run(["make", "-s", "-C", os.path.join(REPO, "examples"), "extrema_hip"], check=True)
    S = 2
    O = pkg.octaves_for(n)
    pyr, rec = tmp_path / "p.f32", tmp_path / "k.bin"
    subprocess.run([exe, str(n), str(S), "lcg:12345", "0", repr(edge_ratio), str(pyr), str(rec)], check=True, timeout=120)
    packed = np.fromfile(pyr, dtype=np.float32)
    assert packed.size == packed_size(n, n, S, O)
    kp = np.fromfile(rec, dtype=pkg.KEYPOINT_DTYPE)
    expect, before = np_extrema(packed, n, n, S, O, edge_ratio=edge_ratio)
    print(f"n = {n}, edge_ratio = {edge_ratio}: {len(expect)} keypoints of {before} extrema")
    assert_sorted(kp)
    assert as_set(kp) == expect
    assert 0 < len(expect) <= before  # the window pyramid has few keypoints: 12 at n = 64, 11 at n = 100
    if n == 64:
        assert (len(expect) < before) == (edge_ratio != 0)  # edge_ratio 10 rejects 3 of the 12
