"""GDP_TUNE_KEEP_SUPPORT: the steady-state kernel (k_keep, csrc/gdp_keep.inc) runs the 4-pixel groups
of the tiles that meet the windows' support as work units of their own, ahead of the tiles, instead
of in serial rounds at the end of those tiles' blocks.

Every combination of the knob (0, 1), the block shape (GDP_TUNE_KEEP_KERNEL 1, 2), the sign map
(GDP_TUNE_KEEP_SIGNS 0, 1) and the input (int32 with negative regions, uint8), on the shapes of
tests/keep_support_cases.py: a build and three rebuilds with different images, every level of every
image equal to the oracle word for word; then the pyramid is poisoned behind the library's back and
one more kept build runs — every word that does not hold the poison is the oracle's, and the set of
words that still hold it is the same for knob 0 and knob 1 (the same stores, from whichever block).
Runs on an MI355X.
"""
import numpy as np
import pytest
from keep_support_cases import SHAPES, span, support_units, tail_units, tiles
from steady_cases import _poison

pytestmark = pytest.mark.gpu

POISON = np.uint32(0xFFFFFFFF)
INT32_MIN = np.iinfo(np.int32).min
N_IMAGES = 4  # per batch entry: the build, two rebuilds, the build over the poison


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


_IMAGES = {}  # (shape, fmt) -> [k][image of the batch]; computed once, never modified
_WANT = {}    # (shape, fmt, k, image) -> the oracle's levels [o * L + s] of the WHOLE image; computed once, never modified


def _images(name, fmt):
    if (name, fmt) not in _IMAGES:
        H, W, _, _, kw = SHAPES[name]
        rng = np.random.default_rng(sum(map(ord, name)) + (fmt == "u8"))
        out = []
        for k in range(N_IMAGES):
            per = []
            for b in range(kw.get("batch", 1)):
                if fmt == "u8":
                    img = rng.integers(0, 256, size=(H, W), dtype=np.int64).astype(np.uint8)
                    img[::7, ::5] = 0
                else:
                    img = rng.integers(1, 2**31 - 1, size=(H, W), dtype=np.int64).astype(np.int32)
                    # negative regions that move from build to build: a band of rows, a band of columns through the
                    # support, and scattered pixels; zeros and INT32_MIN among them
                    r = (k * 37 + b * 11) % H
                    img[r:r + max(1, H // 3)] *= -1
                    c = (k * 211 + b * 64) % W
                    img[:, c:c + max(1, W // 5)] *= -1
                    n = max(4, H * W // 50)
                    img[rng.integers(0, H, n), rng.integers(0, W, n)] = 0
                    img[rng.integers(0, H, n), rng.integers(0, W, n)] = -1
                    img[rng.integers(0, H, n // 4), rng.integers(0, W, n // 4)] = INT32_MIN
                per.append(img)
            out.append(per)
        _IMAGES[(name, fmt)] = out
    return _IMAGES[(name, fmt)]


def _levels(oracle, name, fmt, k, b):
    key = (name, fmt, k, b)
    if key not in _WANT:
        H, W, O, S, _ = SHAPES[name]
        img = _images(name, fmt)[k][b].astype(np.int32)
        lv = oracle.levels(oracle.build_pyramid(img, S, O), H, W, S, O)
        _WANT[key] = [_bits(lv[(o, s)]) for o in range(O) for s in range(S + 3)]
    return _WANT[key]


def _load(ctx, name, imgs):
    r0, r1 = span(name)
    for i, img in enumerate(imgs):
        ctx.set_input(np.ascontiguousarray(img[r0:r1]), i)


def _got(ctx, name):
    """[image][o * L + s]: every level of the context's pyramid as uint32."""
    _, _, O, S, kw = SHAPES[name]
    ctx.sync()
    return [[_bits(ctx.level(b, o, s)) for o in range(O) for s in range(S + 3)] for b in range(kw.get("batch", 1))]


def _want(ctx, oracle, name, fmt, k):
    _, _, O, S, kw = SHAPES[name]
    out = []
    for b in range(kw.get("batch", 1)):
        lv = _levels(oracle, name, fmt, k, b)
        per = []
        for o in range(O):
            rows, _, first = ctx.level_dims(o)
            per += [lv[o * (S + 3) + s][first:first + rows] for s in range(S + 3)]
        out.append(per)
    return out


def _assert_exact(ctx, oracle, name, fmt, k, what):
    for b, (got, want) in enumerate(zip(_got(ctx, name), _want(ctx, oracle, name, fmt, k))):
        for i, (g, w) in enumerate(zip(got, want)):
            assert g.shape == w.shape, (what, b, i, g.shape, w.shape)
            bad = np.flatnonzero(g.ravel() != w.ravel())
            assert bad.size == 0, f"{what} image {b} level {i}: {bad.size} words differ, first at {bad[:5]}"


def _context(pkg, name, fmt, **knobs):
    H, W, O, S, kw = SHAPES[name]
    ctx = pkg.PyramidContext(H, W, S=S, octaves=O, **kw)
    if fmt == "u8":
        ctx.set_input_format("u8")
    ctx.set_tuning(**knobs)
    return ctx


def _run(pkg, oracle, name, fmt, kern, signs, support):
    """The sequence of one knob value; returns the poison maps, [image][level] bool, of the kept build
    right after the first build (with the sign map: the one that writes it) and of a later one (the
    one that skips by it)."""
    imgs = _images(name, fmt)
    what = (name, fmt, kern, signs, support)

    def build(ctx, k, exact=True):
        _load(ctx, name, imgs[k])
        ctx.build()
        assert ctx.tuning()["zeros_clean"] == 1
        if exact:
            _assert_exact(ctx, oracle, name, fmt, k, what + ("build", k))

    def kept_over_poison(ctx, k):
        _poison(ctx)
        build(ctx, k, exact=False)
        held = []
        for got, want in zip(_got(ctx, name), _want(ctx, oracle, name, fmt, k)):
            per = []
            for i, (g, w) in enumerate(zip(got, want)):
                p = g == POISON
                assert (g[~p] == w[~p]).all(), what + ("a stored word is not the oracle's", i)
                per.append(p)
            held.append(per)
        return held

    with _context(pkg, name, fmt, keep_kernel=kern, keep_signs=signs, keep_support=support) as ctx:
        t = ctx.tuning()
        assert t["keep_support"] == support and t["keep_kernel"] == kern
        assert t["keep_support_units"] == (support_units(oracle, name) if support else 0)
        build(ctx, 0)  # the first build stores every byte
        first = kept_over_poison(ctx, 1)
        ctx.pyramid_written()  # the poison: the next build stores every byte again
        for k in (0, 1, 2, 1):  # the full build; kept builds: (the one that writes the map,) the ones that use it
            build(ctx, k)
        return first, kept_over_poison(ctx, 3)


@pytest.mark.parametrize("signs", (0, 1))
@pytest.mark.parametrize("kern", (1, 2))
@pytest.mark.parametrize("fmt", ("i32", "u8"))
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_rebuilds_are_exact_and_the_store_set_does_not_depend_on_the_knob(pkg, oracle, name, fmt, kern, signs):
    runs = [_run(pkg, oracle, name, fmt, kern, signs, support) for support in (0, 1)]
    L = SHAPES[name][3] + 3
    for which, (held0, held1) in enumerate(zip(*runs)):
        some_held = some_stored = False
        for per0, per1 in zip(held0, held1):
            for i, (p0, p1) in enumerate(zip(per0, per1)):
                assert (p0 == p1).all(), (name, fmt, kern, signs, which, "level", divmod(i, L), int((p0 != p1).sum()),
                                          "words differ")
                some_held |= bool(p0.any())
                some_stored |= bool((~p0).any())
        assert some_held and some_stored  # a kept build: stores skipped and stores made


def _units(oracle, name):
    return support_units(oracle, name) + tiles(name) + tail_units(name)


def test_units_knob_counts_the_support_units(pkg, oracle):
    name = "200x1028"
    want = support_units(oracle, name)
    assert want > 3
    with _context(pkg, name, "i32") as ctx:
        t = ctx.tuning()
        assert t["keep_support"] == 1  # the default
        for kern in (1, 2):
            ctx.set_tuning(keep_kernel=kern)
            assert ctx.tuning()["keep_support_units"] == want
        ctx.set_tuning(keep_kernel=0)
        assert ctx.tuning()["keep_support_units"] == 0  # k_build's keep path has no such units
        ctx.set_tuning(keep_kernel=2, keep_support=0)
        assert ctx.tuning()["keep_support_units"] == 0
        ctx.set_tuning(keep_support=1)
        assert ctx.tuning()["keep_support_units"] == want
        lib, _lib = pkg.lib(), __import__(pkg.__name__ + "._lib", fromlist=["_lib"])
        assert lib.gdp_set_tuning(ctx._ctx, _lib.GDP_TUNE_KEEP_SUPPORT_UNITS, want) == _lib.GDP_ERR_ARG  # read-only
        assert lib.gdp_set_tuning(ctx._ctx, _lib.GDP_TUNE_KEEP_SUPPORT, 2) == _lib.GDP_ERR_ARG
        assert ctx.tuning()["keep_support_units"] == want
    with pkg.PyramidContext(200, 1026, S=2, octaves=5) as ctx:  # a width k_keep does not take
        assert ctx.tuning()["keep_support_units"] == 0


@pytest.mark.parametrize("kern", (1, 2))
@pytest.mark.parametrize("cap", ("grid1", "grid3", "grid_sup_minus_1", "plain_stores", "blocks_per_cu1"))
def test_capped_grids_and_plain_stores_rebuild_the_oracle(pkg, oracle, cap, kern):
    name, fmt = "200x1028", "i32"
    sup = support_units(oracle, name)
    knobs = {"grid1": dict(grid=1), "grid3": dict(grid=3), "grid_sup_minus_1": dict(grid=sup - 1),
             "plain_stores": dict(nontemporal=0), "blocks_per_cu1": dict(blocks_per_cu=1)}[cap]
    imgs = _images(name, fmt)
    with _context(pkg, name, fmt, keep_kernel=kern, **knobs) as ctx:
        assert ctx.tuning()["keep_support_units"] == sup
        for k in (0, 1, 2, 3):
            _load(ctx, name, imgs[k])
            ctx.build()
            _assert_exact(ctx, oracle, name, fmt, k, (cap, kern, k))


def test_a_switch_between_kept_builds_leaves_the_flags_and_the_next_build_exact(pkg, oracle):
    name, fmt = "200x1028", "i32"
    imgs = _images(name, fmt)
    with _context(pkg, name, fmt, keep_kernel=1) as ctx:
        for k in (0, 1):
            _load(ctx, name, imgs[k])
            ctx.build()
        t = ctx.tuning()
        assert t["zeros_clean"] == 1 and t["signs_known"] == 1
        for k, support in ((2, 0), (3, 1), (0, 0), (1, 1)):
            ctx.set_tuning(keep_support=support)
            t = ctx.tuning()
            assert t["zeros_clean"] == 1 and t["signs_known"] == 1, (k, support)
            _load(ctx, name, imgs[k])
            ctx.build()
            _assert_exact(ctx, oracle, name, fmt, k, ("switch", k, support))
            t = ctx.tuning()
            assert t["zeros_clean"] == 1 and t["signs_known"] == 1, (k, support)
