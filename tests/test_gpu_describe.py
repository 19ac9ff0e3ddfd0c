"""On-device SIFT descriptors (gdp_describe_keypoints) against the numpy float32 oracle of
tests/describe_oracle.py, which implements the rule of include/gdp.h literally.  The result is a
multiset of 176-byte records and every comparison is of bit patterns.  The oracle is handed the
LIBRARY's tables (gdp_describe_tables: glibc expf and numpy may differ in the last bit).  All cases
run on UPLOADED pyramids, independent of any build kernel, except the state test's and the C++
example's."""
import collections
import ctypes
import functools
import os
import re
import subprocess

import numpy as np
import pytest

from describe_oracle import ORIENTED_DT, as_multiset, assert_download_order, np_describe, oriented_records
from extrema_oracle import (ODD, F, assert_short_downloads, denormal_pyramid, np_extrema, octave_levels, packed_size,
                            small_pipeline, smooth_pyramid, tie_pyramid)
from refine_oracle import extrema_records, records_from_set

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_KINDS = {"tie": tie_pyramid, "smooth": smooth_pyramid}
_TABLES = {}
ANGLES = (0.0, 89.875, 90.0, 359.9)
PER_WAVE = PER_BLOCK = 2  # k_describe: a 32-lane half-wave per record, one wave per block


def tables(pkg, S):
    """({s: the library's W_s}, C, S): what the kernel was given."""
    if S not in _TABLES:
        t = {s: pkg.describe_tables(S, s) for s in range(1, S + 1)}
        _TABLES[S] = ({s: t[s][0] for s in t}, t[1][2], t[1][3])
    return _TABLES[S]


def source(kind, shape):
    return denormal_pyramid(shape, 2 ** 20) if kind == "denormal" else _KINDS[kind](shape)


@functools.lru_cache(maxsize=None)
def oracle_inputs(kind, shape):
    """The oracle's extrema of a shared pyramid as oriented records with seeded angles (the four of
    ANGLES, then random ones): inputs that do not depend on k_extrema, k_refine or k_orient."""
    if kind == "denormal":
        kp = records_from_set(np_extrema(denormal_pyramid(shape, 2 ** 20), *shape)[0])
    else:
        kp = extrema_records(kind, shape)
    out = np.zeros(len(kp), ORIENTED_DT)
    for f in ("octave", "scale", "kind", "row", "col", "value"):
        out[f] = kp[f]
    angle = np.random.default_rng(21).uniform(0, 360, len(kp)).astype(F)
    angle[:len(ANGLES)] = ANGLES
    out["angle"] = np.minimum(angle, np.nextafter(F(360), F(0)))
    out["dscale"], out["drow"], out["dcol"], out["interp"], out["peak"] = 0.25, -0.125, 0.5, 2.5, 3.5  # copied through
    out["bin"], out["peaks"] = np.arange(len(kp)) % 36, 1
    out.setflags(write=False)
    return out


def describe_inputs(pkg, packed, shape, recs, octaves=0):
    H, W, S, O = shape
    with pkg.PyramidContext(H, W, S=S, octaves=octaves) as ctx:
        ctx.upload_pyramid(packed)
        ctx.set_describe_input(recs)
        ctx.describe_keypoints()
        got = ctx.described_keypoints(0)
        assert got.found == ctx.described_count(0) == len(got)
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
        ctx.orient_keypoints()
        ctx.describe_keypoints()  # the same stream, no synchronisation in between
        got = ctx.described_keypoints(0)
        oriented = ctx.oriented_keypoints(0)
        ctx.describe_keypoints()  # the counter is zeroed again
        again = ctx.described_keypoints(0)
        # the oracle's own extrema as the caller's list: clipped windows and rejection, whatever the steps before kept
        ctx.set_describe_input(oracle_inputs(kind, ODD))
        ctx.describe_keypoints()
        direct = ctx.described_keypoints(0)
        ctx.set_describe_input(None)  # back to the oriented list
        ctx.describe_keypoints()
        back = ctx.described_keypoints(0)
    clipped = []
    want, why = np_describe(src, H, W, S, O, oriented, *tables(pkg, S))
    want_direct, why_direct = np_describe(src, H, W, S, O, oracle_inputs(kind, ODD), *tables(pkg, S), clipped_out=clipped)
    print(f"{kind}: {len(oriented)} oriented -> {len(got)} described (oracle {len(want)}); {len(oracle_inputs(kind, ODD))} extrema "
          f"-> {len(direct)} (oracle {len(want_direct)}), {why_direct.count('nonfinite')} rejected, "
          f"{why_direct.count('flat')} flat, {sum(clipped)} clipped")
    assert got.dtype == pkg.DESCRIBED_DTYPE
    assert as_multiset(got) == want and got.found == len(want)
    assert as_multiset(direct) == want_direct and direct.found == len(want_direct)
    assert_download_order(got)
    assert_download_order(direct)
    assert got.tobytes() == again.tobytes() == back.tobytes()  # repeatable, byte for byte
    assert "dropped" not in why and "dropped" not in why_direct
    if kind == "smooth":
        assert len(want) == len(oriented) > 500 and sum(clipped) > 100 and {t[0] for t in want_direct} >= {0, 1, 2, 3}
        assert {t[1] for t in want_direct} == {1, 2, 3}
    if kind == "tie":
        assert why_direct.count("nonfinite") > 50 and 0 < len(want_direct)
    if kind == "denormal":
        assert len(oracle_inputs(kind, ODD)) > 500 and want_direct == []  # gx*gx underflows to +0: flat windows


# ---------------------------------------------------------------------------------------------
# 2. the caller's lists on a 40 x 56 image: every s, two octaves, corners, the angle seams, specials
# ---------------------------------------------------------------------------------------------
def special_pyramid(S, s, seed):
    """A smooth 40 x 56 pyramid of 2 octaves whose levels BELOW s are NaN (they must never be read),
    with one NaN, one inf and a dozen denormals per octave in the levels from s up."""
    H, W, O = 40, 56, 2
    rng = np.random.default_rng(seed)
    p = np.empty(packed_size(H, W, S, O), np.float32)
    for D in octave_levels(p, H, W, S, O):
        rows, cols = D.shape[1:]
        x = rng.standard_normal((S + 3, rows, cols + 4)).astype(F) * F(30.0)
        D[...] = sum(x[:, :, k:k + cols] for k in range(5)) * F(0.2)
        D[:s] = np.nan
        D[rng.integers(s, S + 3), rng.integers(0, rows // 4), rng.integers(0, cols // 4)] = np.nan
        D[rng.integers(s, S + 3), rows - 1 - rng.integers(0, rows // 4), cols - 1 - rng.integers(0, cols // 4)] = np.inf
        for _ in range(12):
            D[rng.integers(s, S + 3), rng.integers(0, rows), rng.integers(0, cols)] = F(rng.integers(-9, 10)) * F(2.0 ** -149)
    return p


def special_points(s, seed):
    rng = np.random.default_rng(seed)
    recs = []
    for o, (rows, cols) in enumerate(((40, 56), (20, 28))):
        pts = [(1, 1), (1, cols - 2), (rows - 2, 1), (rows - 2, cols - 2), (rows // 2, cols // 2)]
        pts += [(int(rng.integers(1, rows - 1)), int(rng.integers(1, cols - 1))) for _ in range(11)]
        angles = list(ANGLES) + [float(F(a)) for a in rng.uniform(0, 360, len(pts))]
        recs.append(oriented_records([(s, r, c, angles[k]) for k, (r, c) in enumerate(pts)], octave=o, kind=-1 if o else 1))
    # the corners once more at the angle seams
    recs.append(oriented_records([(s, 1, 1, 90.0), (s, 38, 54, 359.9), (s, 1, 54, 89.875), (s, 38, 1, 0.0)]))
    return np.concatenate(recs)


@pytest.mark.parametrize("S", [2, 3])
def test_callers_lists_on_a_small_image(pkg, S):
    H, W, O = 40, 56, 2
    seen = collections.Counter()
    with pkg.PyramidContext(H, W, S=S, octaves=O) as ctx:
        for s in range(1, S + 1):
            packed = special_pyramid(S, s, 100 * S + s)
            recs = special_points(s, 7 * S + s)
            ctx.upload_pyramid(packed)
            ctx.set_describe_input(recs)
            ctx.describe_keypoints()
            got = ctx.described_keypoints(0)
            clipped = []
            want, why = np_describe(packed, H, W, S, O, recs, *tables(pkg, S), clipped_out=clipped)
            print(f"S={S} s={s}: {len(recs)} inputs -> {len(got)} described; {collections.Counter(why)}; {sum(clipped)} clipped")
            assert as_multiset(got) == want and got.found == len(want), (S, s)
            assert_download_order(got)
            assert {int(o) for o in got["octave"]} == {0, 1} and sum(clipped) >= 8
            seen.update(why)
            assert all(t[5:10] == tuple(int(F(x).view(np.uint32)) for x in (1.5, 0.25, -0.125, 0.5, 2.5)) for t in want)
    assert seen["ok"] > 20 * S and seen["nonfinite"] > 0 and seen["dropped"] == 0


# ---------------------------------------------------------------------------------------------
# 3. list lengths at the seams of the schedule
# ---------------------------------------------------------------------------------------------
def test_list_lengths_at_the_wave_and_block_seams(pkg):
    H, W, S, O = ODD
    recs = oracle_inputs("smooth", ODD)[:70]
    want_all, why = np_describe(smooth_pyramid(ODD), H, W, S, O, recs, *tables(pkg, S))
    assert why == ["ok"] * len(recs)
    key = lambda r: (int(r["octave"]), int(r["scale"]), int(r["kind"]), int(r["row"]), int(r["col"]))  # noqa: E731
    lengths = sorted({0, 1, PER_WAVE - 1, PER_WAVE, PER_WAVE + 1, PER_BLOCK - 1, PER_BLOCK, PER_BLOCK + 1,
                      2 * PER_BLOCK - 1, 2 * PER_BLOCK, 2 * PER_BLOCK + 1, 63, 64, 65, 70})
    with pkg.PyramidContext(H, W, S=S) as ctx:
        ctx.upload_pyramid(smooth_pyramid(ODD))
        for n in lengths:
            ctx.set_describe_input(recs[:n])  # n = 0: an empty list is a list, not the oriented one
            ctx.describe_keypoints()
            first = {key(r) for r in recs[:n]}
            want = [t for t in want_all if t[:5] in first]  # positions are unique: the outputs of the first n inputs
            got = ctx.described_keypoints(0)
            assert len(want) == n == ctx.described_count(0) and as_multiset(got) == want, n


# ---------------------------------------------------------------------------------------------
# 4. capacity: the counter counts everything, the buffer holds true records only, nothing beyond it
# ---------------------------------------------------------------------------------------------
def raw_records(pkg, ctx, b, n):
    """n records of image b's device buffer, whatever the counter says (test plumbing)."""
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    out = np.zeros(n, pkg.DESCRIBED_DTYPE)
    ctx.sync()
    assert hip.hipMemcpy(out.ctypes.data, ctx.device_described(b)[0], out.nbytes, 2) == 0  # hipMemcpyDeviceToHost (synchronous)
    return out


def want_slice(want, recs):
    keys = {(int(r["octave"]), int(r["scale"]), int(r["kind"]), int(r["row"]), int(r["col"])) for r in recs}
    return sorted(t for t in want if t[:5] in keys)


def plant_oriented(pkg, ctx, recs):
    """Make `recs` image 0's ORIENTED list on the device, counter included: what gdp_orient_keypoints
    would have left (test plumbing; the description reads the list and min(counter, capacity))."""
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    dev, count = ctx.device_oriented(0)
    recs = np.ascontiguousarray(recs, dtype=pkg.ORIENTED_DTYPE)
    n = np.array([len(recs)], np.uint32)
    ctx.sync()
    assert hip.hipMemcpy(dev, recs.ctypes.data, recs.nbytes, 1) == 0  # hipMemcpyHostToDevice (synchronous)
    assert hip.hipMemcpy(count, n.ctypes.data, 4, 1) == 0


def test_capacity_of_eight(pkg):
    """More than eight valid inputs, read from the oriented list: the counter counts all 41, exactly
    eight true records are stored, and image 1's slots, which follow image 0's eight in the buffer,
    keep the bytes they had."""
    H, W, S, O = ODD
    recs = oracle_inputs("smooth", ODD)[:41]
    want, why = np_describe(smooth_pyramid(ODD), H, W, S, O, recs, *tables(pkg, S))
    with pkg.PyramidContext(H, W, S=S, batch=2) as ctx:
        ctx.set_orient_capacity(64)
        ctx.set_describe_capacity(8)
        for b in range(2):
            ctx.upload_pyramid(smooth_pyramid(ODD), b)
        with pytest.raises(pkg.GdpError) as e:  # the caller's lists are bounded by the same capacity
            ctx.set_describe_input(recs[:9])
        assert e.value.status == 1
        ctx.set_describe_input(recs[:0], b=0)
        ctx.set_describe_input(recs[33:41], b=1)
        ctx.describe_keypoints()
        addr = [ctx.device_described(b)[0] for b in range(2)]
        assert addr[1] - addr[0] == 8 * 176
        guard = raw_records(pkg, ctx, 1, 8)
        assert as_multiset(guard) == want_slice(want, recs[33:41])
        ctx.set_describe_input(None, b=0)  # image 0 reads the oriented list; the counter there says 41, the host never reads it
        ctx.set_describe_input(recs[:0], b=1)
        plant_oriented(pkg, ctx, recs)
        ctx.describe_keypoints()
        assert ctx.described_count(0) == 41 and ctx.described_count(1) == 0
        got = ctx.described_keypoints(0)
        assert got.found == 41 and len(got) == 8
        assert_download_order(got)
        stored = raw_records(pkg, ctx, 0, 8)
        after = raw_records(pkg, ctx, 1, 8)
    assert after.tobytes() == guard.tobytes()
    assert as_multiset(stored) == as_multiset(got) and why == ["ok"] * 41
    assert not collections.Counter(as_multiset(stored)) - collections.Counter(want) and len(set(as_multiset(stored))) == 8


# ---------------------------------------------------------------------------------------------
# 5. batch of 3: the oriented list, a caller's list and an empty list side by side
# ---------------------------------------------------------------------------------------------
def test_batch_of_three_with_different_lists(pkg):
    H, W, S, O = ODD
    own = oracle_inputs("tie", ODD)[:100]
    with pkg.PyramidContext(H, W, S=S, batch=3) as ctx:
        ctx.upload_pyramid(smooth_pyramid(ODD), 0)
        ctx.upload_pyramid(tie_pyramid(ODD), 1)
        ctx.upload_pyramid(smooth_pyramid(ODD), 2)
        ctx.detect_extrema()
        ctx.refine_keypoints()
        ctx.orient_keypoints()
        ctx.set_describe_input(own, b=1)  # image 0 keeps the oriented list
        ctx.set_describe_input(own[:0], b=2)
        ctx.describe_keypoints()
        got = [ctx.described_keypoints(b) for b in range(3)]
        oriented = [ctx.oriented_keypoints(b) for b in range(3)]
        addr = [ctx.device_described(b)[0] for b in range(3)]
        assert addr[1] - addr[0] == addr[2] - addr[1] == 2 * 65536 * 176  # capacity 0: the orientation object's
    assert as_multiset(got[0]) == np_describe(smooth_pyramid(ODD), H, W, S, O, oriented[0], *tables(pkg, S))[0]
    assert as_multiset(got[1]) == np_describe(tie_pyramid(ODD), H, W, S, O, own, *tables(pkg, S))[0]
    assert len(got[0]) > 500 and 0 < len(got[1]) <= 100 and len(oriented[2]) > 500 and len(got[2]) == 0 == got[2].found


# ---------------------------------------------------------------------------------------------
# 6. state: the description only reads the context and the orientation object
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
        state = lambda: (ctx.checksum(0), ctx.keypoints(0).tobytes(), ctx.refined_keypoints(0).tobytes(),  # noqa: E731
                         ctx.oriented_keypoints(0).tobytes(), ctx.pyramid(0).tobytes())
        before = state()
        ctx.describe_keypoints()
        got = ctx.described_keypoints(0)
        assert ctx.tuning()["zeros_clean"] == 1  # the next build is still the steady-state one
        assert state() == before and len(before[3]) > 0
        want, why = np_describe(ctx.pyramid(0), n, n, S, ctx.O, ctx.oriented_keypoints(0), *tables(pkg, S))
        assert as_multiset(got) == want and len(want) > 0
        ctx.build()
        assert ctx.tuning()["zeros_clean"] == 1 and ctx.checksum(0) == before[0]
        ctx.describe_keypoints()
        assert ctx.described_keypoints(0).tobytes() == got.tobytes()


# ---------------------------------------------------------------------------------------------
# 7. refusals
# ---------------------------------------------------------------------------------------------
def test_refused_contexts_and_inputs(pkg):
    L = pkg.lib()
    with pkg.PyramidContext(64, 64, S=2, octaves=5, row_begin=0, row_end=32) as ctx:
        w = ctypes.c_void_p()
        assert L.gdp_describe_create(ctypes.byref(w), ctx._ctx, None, 0) == 3 and w.value is None  # a row band
        assert b"band" in L.gdp_describe_last_error(None)
        with pytest.raises(pkg.GdpError) as e:
            ctx.describe_keypoints()
        assert e.value.status == 3 and "band" in str(e.value)
    S, rows, cols = 2, 16, 24
    good = oriented_records([(1, 1, 1, 0.0), (2, 6, 11, 123.5), (S, rows - 2, cols - 2, 359.75)])
    with pkg.PyramidContext(rows, cols, S=S, octaves=2) as ctx:
        ctx.upload_pyramid(np.zeros(ctx.packed_floats(), np.float32))
        # no orientation object and no list of the caller's
        w = ctypes.c_void_p()
        assert L.gdp_describe_create(ctypes.byref(w), ctx._ctx, None, 0) == 0
        try:
            assert L.gdp_describe_keypoints(w, None) == 3 and b"no input list" in L.gdp_describe_last_error(w)
            rec = np.ascontiguousarray(good, dtype=pkg.ORIENTED_DTYPE)
            assert L.gdp_describe_set_input(w, 0, ctypes.c_void_p(rec.ctypes.data), 3) == 0
            assert L.gdp_describe_keypoints(w, None) == 0  # a list of the caller's is enough
            found = ctypes.c_size_t(7)
            assert L.gdp_described_count(w, 0, ctypes.byref(found)) == 0 and found.value == 0  # flat windows
            assert L.gdp_describe_set_input(w, 0, None, 0) == 0  # back to src's list, which does not exist
            assert L.gdp_describe_keypoints(w, None) == 3
        finally:
            L.gdp_describe_destroy(w)
        assert ctx.described_count(0) == 0 and len(ctx.described_keypoints(0)) == 0
        ctx.set_describe_capacity(4)
        ctx.set_describe_input(good)
        bad = []
        for field, value in [("scale", 0), ("scale", S + 1), ("row", 0), ("row", rows - 1), ("col", 0), ("col", cols - 1),
                             ("octave", 2), ("angle", 360.0), ("angle", -0.125), ("angle", np.nan), ("angle", np.inf)]:
            r = good.copy()
            r[field][1] = value
            bad.append(r)
        bad.append(oriented_records([(1, 7, 5, 0.0)], octave=1))  # row 7 is the last row of octave 1 (8 x 12)
        bad.append(oriented_records([(1, 2, 2, 0.0)] * 5))  # n above the capacity
        for r in bad:
            with pytest.raises(pkg.GdpError) as e:
                ctx.set_describe_input(r)
            assert e.value.status == 1
        # a refused list changed nothing: the good one is still image 0's
        ctx.upload_pyramid(np.arange(ctx.packed_floats(), dtype=np.float32) % 7)
        ctx.describe_keypoints()
        got = ctx.described_keypoints(0)
        want, _ = np_describe(np.arange(ctx.packed_floats(), dtype=np.float32) % 7, rows, cols, S, 2, good, *tables(pkg, S))
        assert as_multiset(got) == want and len(want) == 3


# ---------------------------------------------------------------------------------------------
# 8. the C++ example, executed
# ---------------------------------------------------------------------------------------------
def test_cpp_example_matches_the_python_path(pkg, oracle):
    exe = os.path.join(REPO, "examples", "describe_hip")
    if not os.path.exists(exe):
        subprocess.run(["make", "-s", "-C", os.path.join(REPO, "examples"), "describe_hip"], check=True)
    n, S, seed = 64, 2, 12345
    out = subprocess.run([exe, str(n), str(S), f"lcg:{seed}", "0.5", "10"], check=True, timeout=120, capture_output=True,
                         text=True).stdout
    m = re.match(r"(\d+) keypoints, (\d+) refined, (\d+) oriented, (\d+) described\n", out)
    assert m, out
    g = pkg.GaussPyramid(oracle.lcg_image(n, n, seed), n, S)
    try:
        g.GenerateDoG()
        kp = g.DetectExtrema()
        rf = g.RefineKeypoints(0.5, 10.0)
        ok = g.OrientKeypoints()
        de = g.DescribeKeypoints()
        want, _ = np_describe(g.pyramid(), n, n, S, g.layer, ok, *tables(pkg, S))
    finally:
        g.close()
    print(out)
    assert tuple(int(x) for x in m.groups()) == (len(kp), len(rf), len(ok), len(de)) and len(de) > 0
    assert as_multiset(de) == want
    lines = re.findall(r"^octave (\d+) scale (\d+) sample \((\d+), (\d+)\) angle (\S+) bin (\d+) desc ([0-9a-f]{256})$", out, re.M)
    assert len(lines) == min(len(de), 8)
    for line, k in zip(lines, de):
        assert line == (str(k["octave"]), str(k["scale"]), str(k["row"]), str(k["col"]), "%.4f" % k["angle"], str(k["bin"]),
                        bytes(k["desc"]).hex())


# ---------------------------------------------------------------------------------------------
# 9. the list handling's edges on the small image
# ---------------------------------------------------------------------------------------------
def test_short_downloads_and_an_empty_list_then_none(pkg, oracle):
    L = pkg.lib()
    with small_pipeline(pkg, oracle, 4) as ctx:
        full = ctx.described_keypoints(0)
        assert_short_downloads(lambda *a: L.gdp_download_described(ctx._describe, 0, *a), full)
        ctx.set_describe_input(np.zeros(0, pkg.ORIENTED_DTYPE))
        ctx.describe_keypoints()
        assert ctx.described_count(0) == 0 and len(ctx.described_keypoints(0)) == 0
        ctx.set_describe_input(None)  # the oriented list again
        ctx.describe_keypoints()
        assert ctx.described_keypoints(0).tobytes() == full.tobytes()
