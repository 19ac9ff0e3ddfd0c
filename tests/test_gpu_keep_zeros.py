"""GDP_TUNE_KEEP_ZEROS: a build on a clean context-owned pyramid skips the DoG stores outside the
windows' support (they are +0 for any input and an earlier build already stored them).

Every comparison is bitwise on uint32 views (-0 != +0 matters: level S+2 outside the support is
copysign(0, x)), against the oracle or against a fresh context built with keep_zeros = 0 — never
against another kept build alone.  Shapes: 512 x 512 x 5 octaves (octaves 0-2 mostly outside the
support, octave 4 wholly inside, support edges not multiples of 4), 203 x 331 (cols & 3 != 0 in
several octaves: the partial-store path), a row band, batch 3, uint8 input.  Runs on an MI355X.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

S, L = 2, 5
POISON = np.uint32(0xFFFFFFFF)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _assert_same(got, want, what):
    g, w = _bits(got).ravel(), _bits(want).ravel()
    assert g.shape == w.shape, (what, g.shape, w.shape)
    bad = np.flatnonzero(g != w)
    assert bad.size == 0, f"{what}: {bad.size} words differ, first at {bad[:5]}: {g[bad[:5]]} vs {w[bad[:5]]}"


def _flip(img, seed):
    """`img` with the opposite sign over large areas, and a scattering of zeros."""
    out = -img
    rng = np.random.default_rng(seed)
    out[rng.integers(0, img.shape[0], 400), rng.integers(0, img.shape[1], 400)] = 0
    return out


def _images(oracle, H, W, seed=12345):
    """(A, B): A positive on top, negative below, some zeros; B the other way round."""
    a = oracle.lcg_image(H, W, seed)
    a[H // 2:] *= -1
    a[::7, ::5] = 0
    return a, _flip(a, H + W)


def _support(oracle, H, W, O):
    """Per octave: (rows, cols) boolean masks of the window support — some tap of some scale,
    under either window centre, is non-zero."""
    out = []
    for o in range(O):
        masks = []
        for n in (H, W):
            m = np.zeros(n >> o, bool)
            for centre in ("serial", "intlen"):
                for s in range(L):
                    t = oracle.taps(n, o, s, centre)[:n >> o]
                    m[:t.size] |= t != 0
            masks.append(m)
        out.append(tuple(masks))
    return out


def _skipped(oracle, H, W, O, dims=None):
    """Per octave, the pixels whose DoG stores a kept build skips: rows outside the row support,
    and 4-pixel groups wholly outside the column support.  `dims`: a band context's level_dims
    per octave (rows held, cols, first global row); None = the whole image."""
    out = []
    for o, (rows, cols) in enumerate(_support(oracle, H, W, O)):
        n = cols.size
        grp = np.zeros(n, bool)
        for c in range(0, n, 4):
            grp[c:c + 4] = not cols[c:c + 4].any()
        nrows, _, first = dims[o] if dims else (H >> o, n, 0)
        out.append(~rows[first:first + nrows, None] | grp[None, :])
    return out


@pytest.fixture(scope="module")
def sq(oracle):
    """The 512^2 pair and their oracle pyramids (5 octaves), shared and never modified."""
    H = W = 512
    a, b = _images(oracle, H, W)
    want = {k: oracle.build_pyramid(v, S, 5) for k, v in (("a", a), ("b", b))}
    for v in want.values():
        v.setflags(write=False)
    sk = _skipped(oracle, H, W, 5)
    # the shape does what the test needs: octaves 0-2 mostly outside, octave 4 wholly inside
    assert all(sk[o].mean() > 0.5 for o in range(3)) and not sk[4].any()
    return {"H": H, "W": W, "O": 5, "a": a, "b": b, "want": want, "skipped": sk}


def _clean(ctx):
    return ctx.tuning()["zeros_clean"]


def test_fresh_full_build_is_the_oracle(pkg, oracle, sq):
    """The reference of the tests below: keep_zeros = 0 on a fresh context gives the oracle's bits."""
    with pkg.PyramidContext(sq["H"], sq["W"], S=S, octaves=sq["O"]) as ctx:
        ctx.set_tuning(keep_zeros=0)
        assert ctx.tuning()["keep_zeros"] == 0 and _clean(ctx) == 0
        ctx.set_input(sq["b"])
        ctx.build()
        ctx.sync()
        _assert_same(ctx.pyramid(0), sq["want"]["b"], "fresh full build")
    with pkg.PyramidContext(sq["H"], sq["W"], S=S, octaves=sq["O"]) as ctx:
        assert ctx.tuning()["keep_zeros"] == 1  # the default


@pytest.mark.parametrize("zw", [0, 1])
def test_rebuild_equals_fresh_build_every_variant(pkg, sq, zw):
    """Image A then image B on one context, every build variant, both zero-window modes: the second
    (kept) build equals the oracle's build of B in every level."""
    for v in pkg.build_variants():
        with pkg.PyramidContext(sq["H"], sq["W"], S=S, octaves=sq["O"]) as ctx:
            ctx.set_tuning(variant=v, zero_window=zw)
            ctx.set_input(sq["a"])
            ctx.build()
            assert _clean(ctx) == 1, (v, zw)
            ctx.set_input(sq["b"])
            assert _clean(ctx) == 1, (v, zw)  # a new input leaves the pyramid alone
            ctx.build()
            ctx.sync()
            _assert_same(ctx.pyramid(0), sq["want"]["b"], ("kept rebuild", v, zw))
            assert _clean(ctx) == 1


def _band_want(oracle, ctx, want, H, W, O, b=0):
    lv = oracle.levels(want, H, W, S, O)
    out = []
    for o in range(O):
        rows, _, first = ctx.level_dims(o)
        out += [lv[(o, s)][first:first + rows] for s in range(L)]
    return out


@pytest.mark.parametrize("case", ["203x331", "band", "batch3", "u8"])
def test_rebuild_other_shapes(pkg, oracle, sq, case):
    """The same on a non-square image with ragged rows, a row band, a batch and uint8 input; the
    fresh keep_zeros = 0 build of the same context type is compared with the oracle too."""
    kw, O, fmt = {}, 0, np.int32
    H, W = sq["H"], sq["W"]
    if case == "203x331":
        H, W = 203, 331
        firsts = list(_images(oracle, H, W, 99))
    elif case == "band":
        kw, O = dict(row_begin=128, row_end=384), 5
        firsts = [sq["a"], sq["b"]]
    elif case == "batch3":
        kw, O = dict(batch=3), 5
        firsts = [sq["a"], sq["b"]]
    else:
        kw, O, fmt = dict(input_format="u8"), 5, np.uint8
        a = (oracle.lcg_image(H, W, 5) & 0xFF).astype(np.uint8)
        b = (255 - a).astype(np.uint8)
        b[::3, ::11] = 0
        firsts = [a, b]
    Oo = O or oracle.default_octaves(H, W)
    B = kw.get("batch", 1)
    r0, r1 = kw.get("row_begin", 0), kw.get("row_end", H)
    # image i of the batch in build k: alternate the pair so every image changes sign between builds
    seq = [[firsts[(k + i) % 2] for i in range(B)] for k in range(2)]
    wants = [oracle.build_pyramid(np.asarray(im, np.int32), S, Oo) for im in seq[1]]
    for keep in (0, 1):
        with pkg.PyramidContext(H, W, S=S, octaves=O, **kw) as ctx:
            assert ctx.O == Oo
            ctx.set_tuning(keep_zeros=keep)
            for k in range(2):
                for i in range(B):
                    ctx.set_input(np.ascontiguousarray(seq[k][i][r0:r1], dtype=fmt), i)
                if k == 1:
                    assert _clean(ctx) == 1
                ctx.build()
            ctx.sync()
            for i in range(B):
                if case == "band":
                    got = [ctx.level(i, o, s) for o in range(Oo) for s in range(L)]
                    for g, w in zip(got, _band_want(oracle, ctx, wants[i], H, W, Oo)):
                        _assert_same(g, w, (case, keep, i))
                else:
                    _assert_same(ctx.pyramid(i), wants[i], (case, keep, i))


def _poison(ctx):
    """0xFF over the whole context-owned pyramid, behind the library's back."""
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemset.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t]
    hip.hipDeviceSynchronize.argtypes = []
    ctx.sync()
    assert hip.hipMemset(ctypes.c_void_p(ctx.device_level_ptr(0, 0, 0)), 0xFF, ctx.pyramid_bytes()) == 0
    assert hip.hipDeviceSynchronize() == 0


@pytest.mark.parametrize("shape", ["512", "203x331", "band"])
@pytest.mark.parametrize("keep", [1, 0])
def test_poison_survives_only_where_the_stores_are_skipped(pkg, oracle, sq, shape, keep):
    """After a build, the pyramid is overwritten with 0xFF bytes behind the library's back.  The
    next build (keep_zeros = 1) leaves the poison exactly in the DoG levels outside the support and
    writes level S+2 and everything inside the support correctly; gdp_pyramid_written then makes
    the following build store everything.  With keep_zeros = 0 the first rebuild already does."""
    kw = {}
    if shape == "203x331":
        H, W, O = 203, 331, 0
        a, b = _images(oracle, H, W, 99)
    else:
        H, W, O, a, b = sq["H"], sq["W"], sq["O"], sq["a"], sq["b"]
        if shape == "band":
            kw = dict(row_begin=128, row_end=384)
    Oo = O or oracle.default_octaves(H, W)
    r0, r1 = kw.get("row_begin", 0), kw.get("row_end", H)
    with pkg.PyramidContext(H, W, S=S, octaves=O, **kw) as ctx:
        skipped = _skipped(oracle, H, W, Oo, [ctx.level_dims(o) for o in range(Oo)])
        ctx.set_tuning(keep_zeros=keep)
        ctx.set_input(a[r0:r1])
        ctx.build()
        _poison(ctx)
        assert _clean(ctx) == 1  # nobody told the library
        ctx.set_input(b[r0:r1])
        ctx.build()
        ctx.sync()
        want = _band_want(oracle, ctx, oracle.build_pyramid(b, S, Oo), H, W, Oo)
        n_poison = 0
        for o in range(Oo):
            for s in range(L):
                got, w = _bits(ctx.level(0, o, s)), _bits(want[o * L + s])
                if keep and s < L - 1:
                    sk = skipped[o]
                    assert sk.shape == got.shape, (o, sk.shape, got.shape)
                    assert (got[sk] == POISON).all(), ("a skipped store was made", o, s)
                    assert (w[sk] == 0).all()  # what an earlier build would have left there: +0
                    _assert_same(got[~sk], w[~sk], ("inside the support", o, s))
                    n_poison += int(sk.sum())
                else:
                    _assert_same(got, w, ("stored level", o, s, keep))
        assert (n_poison > 0) == bool(keep)
        ctx.pyramid_written(-1)
        assert _clean(ctx) == 0
        ctx.build()
        ctx.sync()
        for o in range(Oo):
            for s in range(L):
                _assert_same(ctx.level(0, o, s), want[o * L + s], ("after pyramid_written", o, s))
        assert _clean(ctx) == 1


def _nan_level(ctx, o=0):
    rows, cols, _ = ctx.level_dims(o)
    return np.full((rows, cols), np.nan, np.float32)


def _mirrored(pkg, ctx):
    """gdp_generate_dog_mirrored (the drop-in classes' GenerateDoG on a mirrored GaussPy) of a
    NaN-filled host mirror."""
    lib = pkg.lib()
    n = lib.gdp_image_floats(ctx._ctx)
    hptr = ctypes.c_void_p()
    assert lib.gdp_host_alloc(n * 4, ctypes.byref(hptr)) == 0
    try:
        host = np.ctypeslib.as_array(ctypes.cast(hptr, ctypes.POINTER(ctypes.c_float)), shape=(n,))
        host[:] = np.nan
        assert lib.gdp_generate_dog_mirrored(ctx._ctx, 0, hptr) == 0
    finally:
        lib.gdp_host_free(hptr)


MUTATORS = {
    "upload_level": lambda pkg, c: c.upload_level(0, 0, 1, _nan_level(c)),
    "upload_pyramid": lambda pkg, c: c.upload_pyramid(np.full(c.packed_floats(), np.nan, np.float32)),
    "init": lambda pkg, c: c.init(),
    "gauss_range": lambda pkg, c: c.gauss_range(0, c.O),
    "dog_range": lambda pkg, c: c.dog_range(0, c.O),
    "generate_dog": lambda pkg, c: c.generate_dog(),
    "build_subset": lambda pkg, c: c.build_subset(),
    "build_gaussian": lambda pkg, c: c.build_gaussian(),
    "mirrored_generate_dog": _mirrored,
    "pyramid_written_one_image": lambda pkg, c: c.pyramid_written(0),
}


@pytest.mark.parametrize("name", sorted(MUTATORS))
def test_every_mutator_invalidates(pkg, sq, name):
    """build, the mutator, ZEROS_CLEAN == 0, build: the result is the oracle's build."""
    with pkg.PyramidContext(sq["H"], sq["W"], S=S, octaves=sq["O"]) as ctx:
        ctx.set_input(sq["a"])
        ctx.build()
        assert _clean(ctx) == 1
        MUTATORS[name](pkg, ctx)
        assert _clean(ctx) == 0, name
        ctx.set_input(sq["b"])
        ctx.build()
        ctx.sync()
        _assert_same(ctx.pyramid(0), sq["want"]["b"], ("after", name))
        assert _clean(ctx) == 1


def test_set_window_centre_invalidates(pkg, oracle, sq):
    with pkg.PyramidContext(sq["H"], sq["W"], S=S, octaves=sq["O"]) as ctx:
        ctx.set_input(sq["a"])
        ctx.build()
        assert _clean(ctx) == 1
        ctx.set_window_centre("intlen")
        assert _clean(ctx) == 0
        ctx.set_input(sq["b"])
        ctx.build()
        ctx.sync()
        _assert_same(ctx.pyramid(0), oracle.build_pyramid(sq["b"], S, sq["O"], centre="intlen"), "intlen")


def test_copy_band_invalidates_the_band_context(pkg, oracle, sq):
    H, W, O = sq["H"], sq["W"], sq["O"]
    with pkg.PyramidContext(H, W, S=S, octaves=O) as full, \
            pkg.PyramidContext(H, W, S=S, octaves=O, row_begin=128, row_end=384) as band:
        full.upload_pyramid(np.full(full.packed_floats(), np.nan, np.float32))
        band.set_input(sq["a"][128:384])
        band.build()
        assert _clean(band) == 1
        band.copy_band_from(full)
        assert _clean(band) == 0
        band.set_input(sq["b"][128:384])
        band.build()
        band.sync()
        got = [band.level(0, o, s) for o in range(O) for s in range(L)]
        for g, w in zip(got, _band_want(oracle, band, sq["want"]["b"], H, W, O)):
            _assert_same(g, w, "band after copy_band")


def test_caller_bound_output_is_never_kept(pkg, oracle, sq):
    """Binding and unbinding a caller tensor both invalidate; while it is bound ZEROS_CLEAN never
    becomes 1 and every build overwrites all of the caller's NaNs."""
    import torch

    H, W, O = sq["H"], sq["W"], sq["O"]
    want = oracle.levels(sq["want"]["b"], H, W, S, O)
    with pkg.PyramidContext(H, W, S=S, octaves=O) as ctx:
        ctx.set_input(sq["a"])
        ctx.build()
        assert _clean(ctx) == 1
        buf = torch.full((ctx.pyramid_bytes() // 4,), float("nan"), device="cuda")
        ctx.bind_device_output(buf.data_ptr(), ctx.pyramid_bytes(), keepalive=buf)
        assert _clean(ctx) == 0
        ctx.set_input(sq["b"])
        for _ in range(2):
            ctx.build()
            ctx.sync()
            assert _clean(ctx) == 0
            host = buf.cpu().numpy()
            for (o, s), lev in want.items():
                off = ctx.level_offset(0, o, s)
                _assert_same(host[off:off + lev.size], lev, ("bound", o, s))
            buf.fill_(float("nan"))
            torch.cuda.synchronize()
        ctx.unbind_device_output()
        assert _clean(ctx) == 0
        ctx.build()
        ctx.sync()
        _assert_same(ctx.pyramid(0), sq["want"]["b"], "own pyramid after unbind")
        assert _clean(ctx) == 1


def test_time_builds_and_autotune_leave_a_correct_pyramid(pkg, sq):
    """The build timers run an untimed build first (every timed launch in the same clean state) and
    leave the oracle's bits, whatever the pyramid held."""
    with pkg.PyramidContext(sq["H"], sq["W"], S=S, octaves=sq["O"]) as ctx:
        ctx.set_input(sq["b"])
        ctx.upload_pyramid(np.full(ctx.packed_floats(), np.nan, np.float32))
        assert ctx.time_builds(2) > 0
        _assert_same(ctx.pyramid(0), sq["want"]["b"], "time_builds")
        assert _clean(ctx) == 1
        ctx.upload_pyramid(np.full(ctx.packed_floats(), np.nan, np.float32))
        ctx.autotune(iters=1)
        _assert_same(ctx.pyramid(0), sq["want"]["b"], "autotune")
