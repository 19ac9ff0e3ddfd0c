"""GDP_TUNE_KEEP_SIGNS: the steady-state kernel (k_keep, csrc/gdp_keep.inc) skips its level-S+2
stores where they would put +0 over +0.

Outside the windows' support k_keep owes level S+2 = copysign(0, x).  The context keeps a sign map
on the device, one byte per input row of a 16 x 256 tile, that only int32 k_keep launches write:
the first one after anything invalidating (GDP_TUNE_SIGNS_KNOWN = 0) stores everything and
establishes the map; from then on a row segment whose pixels are all non-negative now, and were at
the build before, stores nothing in any fused octave.

Every comparison is bitwise on uint32 views against the oracle, every level of every image after
every build.  The sequences: non-negative x 3 (full build, establishing build, skipping build), one
negative pixel (its row segment stores again), non-negative x 2 (the first restores +0 over the -0,
the second skips again) — with the negative pixel at every seam of the kernel's indexing.  The
store-map tests overwrite the pyramid behind the library's back and find the poison exactly on the
words whose stores the model says were skipped.  Runs on an MI355X.
"""
import numpy as np
import pytest
from steady_cases import FUSED, TILE_COLS, TILE_ROWS, _poison, _support

pytestmark = pytest.mark.gpu

POISON = np.uint32(0xFFFFFFFF)
KERNELS = (1, 2)  # GDP_TUNE_KEEP_KERNEL values that select k_keep (4 / 2 rows per wave)
INT32_MIN = np.iinfo(np.int32).min

# name: H, W, octaves, S, context keywords
SHAPES = {
    "200x1028": (200, 1028, 5, 2, {}),        # H % 16 != 0, a last tile column of one 4-pixel group
    "64x2048_o7": (64, 2048, 7, 2, {}),       # tail units (octaves 5 and 6)
    "96x768_b3": (96, 768, 3, 2, dict(batch=3)),
    "96x768_b3_s0": (96, 768, 3, 0, dict(batch=3)),
    "96x768_b3_s3": (96, 768, 3, 3, dict(batch=3)),
    "band_lo": (1024, 512, 5, 2, dict(row_begin=0, row_end=512)),
    "band_hi": (1024, 512, 5, 2, dict(row_begin=512, row_end=1024)),
    "8x512": (8, 512, 0, 2, {}),              # less than one tile row
}

# (shape, image of the batch, global row, column, value) of the one negative pixel, by name
PIXELS = {
    "tile_first_col": ("200x1028", 0, 150, 256, -1),
    "tile_last_col": ("200x1028", 0, 20, 255, -7),
    "partial_tile_last_col": ("200x1028", 0, 10, 1027, -1),
    "row0": ("200x1028", 0, 0, 300, -3),
    "odd_row": ("200x1028", 0, 37, 900, -1),          # reaches octave 0 only
    "all_octaves": ("200x1028", 0, 48, 512 + 256, -1),  # (16 k, 16 m): reaches all five octaves
    "last_row": ("200x1028", 0, 199, 5, -1),          # H % 16 != 0: the last tile row is partial
    "int32_min": ("200x1028", 0, 160, 16, INT32_MIN),
    "tail_shape": ("64x2048_o7", 0, 16, 1024 + 512, -1),
    "image2": ("96x768_b3", 2, 32, 700, -1),
    "image2_s0": ("96x768_b3_s0", 2, 80, 4, -1),
    "image2_s3": ("96x768_b3_s3", 2, 0, 767, -1),
    "band_lo_last_row": ("band_lo", 0, 511, 511, -1),
    "band_hi_first_row": ("band_hi", 0, 512, 256, -1),
    "short_tile": ("8x512", 0, 7, 511, -1),
}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _assert_bits(g, w, what):
    """uint32 views, word for word."""
    assert g.dtype == np.uint32 and w.dtype == np.uint32
    g, w = g.ravel(), w.ravel()
    assert g.shape == w.shape, (what, g.shape, w.shape)
    bad = np.flatnonzero(g != w)
    assert bad.size == 0, f"{what}: {bad.size} words differ, first at {bad[:5]}: {g[bad[:5]]} vs {w[bad[:5]]}"


def _octaves(oracle, name):
    H, W, O, _, _ = SHAPES[name]
    return O or oracle.default_octaves(H, W)


_NONNEG = {}  # shape -> (P, Q): two non-negative images per batch entry, with zeros; computed once, never modified
_WANT = {}    # (shape, image key) -> the oracle's levels [o * L + s] of the WHOLE image; computed once, never modified


def _nonneg(oracle, name):
    if name not in _NONNEG:
        H, W, _, _, kw = SHAPES[name]
        pair = []
        for k in range(2):
            per = []
            for i in range(kw.get("batch", 1)):
                img = np.abs(oracle.lcg_image(H, W, 1000 + 10 * k + i)).astype(np.int32)
                img[img < 0] = 0  # |INT32_MIN|
                img[::5, ::3] = 0
                per.append(img)
            pair.append(per)
        _NONNEG[name] = pair
    return _NONNEG[name]


def _levels(oracle, name, key, img):
    if (name, key) not in _WANT:
        H, W, _, S, _ = SHAPES[name]
        O = _octaves(oracle, name)
        lv = oracle.levels(oracle.build_pyramid(np.asarray(img, np.int32), S, O), H, W, S, O)
        _WANT[(name, key)] = [lv[(o, s)] for o in range(O) for s in range(S + 3)]
    return _WANT[(name, key)]


def _cut(ctx, want, o, s, L):
    rows, _, first = ctx.level_dims(o)
    return want[o * L + s][first:first + rows]


def _check(ctx, oracle, name, keys_imgs, what):
    """Every level of every image of the batch against the oracle's (cut to the context's rows)."""
    _, _, _, S, _ = SHAPES[name]
    L, O = S + 3, _octaves(oracle, name)
    ctx.sync()
    for i, (key, img) in enumerate(keys_imgs):
        want = _levels(oracle, name, key, img)
        for o in range(O):
            for s in range(L):
                _assert_bits(_bits(ctx.level(i, o, s)), _bits(_cut(ctx, want, o, s, L)), (what, i, o, s))


def _load(ctx, name, imgs):
    H, kw = SHAPES[name][0], SHAPES[name][4]
    r0, r1 = kw.get("row_begin", 0), kw.get("row_end", H)
    for i, img in enumerate(imgs):
        ctx.set_input(np.ascontiguousarray(img[r0:r1]), i)


def _with_pixel(base, b, r, c, v):
    out = [im for im in base]
    out[b] = base[b].copy()
    out[b][r, c] = v
    return out


def _known(ctx):
    return ctx.tuning()["signs_known"]


@pytest.mark.parametrize("kern", KERNELS)
@pytest.mark.parametrize("pixel", sorted(PIXELS))
def test_one_negative_pixel_stores_its_row_and_the_next_build_restores_it(pkg, oracle, pixel, kern):
    name, b, r, c, v = PIXELS[pixel]
    H, W, O, S, kw = SHAPES[name]
    P, Q = _nonneg(oracle, name)
    N = _with_pixel(Q, b, r, c, v)
    B = len(P)
    keyP = [(("P", i), P[i]) for i in range(B)]
    keyQ = [(("Q", i), Q[i]) for i in range(B)]
    keyN = [((("N", pixel) if i == b else ("Q", i)), N[i]) for i in range(B)]
    # full build, establishing build, skipping build, the pixel, the restoring build, skipping again
    seq = [(P, keyP, 0), (Q, keyQ, 1), (P, keyP, 1), (N, keyN, 1), (P, keyP, 1), (Q, keyQ, 1)]
    with pkg.PyramidContext(H, W, S=S, octaves=O, **kw) as ctx:
        ctx.set_tuning(keep_kernel=kern)
        assert ctx.tuning()["keep_signs"] == 1 and _known(ctx) == 0
        for k, (imgs, keys, known) in enumerate(seq):
            _load(ctx, name, imgs)
            ctx.build()
            assert _known(ctx) == known, (pixel, kern, k)
            _check(ctx, oracle, name, keys, (pixel, kern, k))


# ---------------------------------------------------------------------------------------------
# the store map
# ---------------------------------------------------------------------------------------------
def _fast_masks(oracle, ctx, name):
    """Per fused octave, the words of level S+2 (of the rows the context holds) that k_keep stores
    from registers: the (tile, octave) pairs whose footprint misses the support's bounding ranges
    (the hit test of steady_cases.clean_tiles, restated per word)."""
    H, W, _, S, kw = SHAPES[name]
    O = _octaves(oracle, name)
    r0, r1 = kw.get("row_begin", 0), kw.get("row_end", H)
    sup = _support(oracle, H, W, O, S)
    out = []
    for o in range(min(O, FUSED)):
        box = []
        for m in sup[o]:
            nz = np.flatnonzero(m)
            box.append((int(nz[0]), int(nz[-1]) + 1) if nz.size else (0, 0))
        (sr0, sr1), (sc0, sc1) = box
        rows, cols, first = ctx.level_dims(o)
        assert first == r0 >> o
        mask = np.zeros((rows, cols), bool)
        for tr in range(-(-(r1 - r0) // TILE_ROWS)):
            for tc in range(-(-W // TILE_COLS)):
                l_lo = tr * TILE_ROWS >> o  # local row of the level
                r_lo, r_hi = first + l_lo, first + l_lo + (TILE_ROWS >> o)
                c_lo = tc * TILE_COLS >> o
                c_hi = min(c_lo + (TILE_COLS >> o), W >> o)
                if not (r_lo < sr1 and r_hi > sr0 and c_lo < sc1 and c_hi > sc0):
                    mask[l_lo:l_lo + (TILE_ROWS >> o), c_lo:c_hi] = True
        out.append(mask)
    return out


def _row_segment(masks, ctx, name, r, c):
    """Per fused octave, the words sourced from the row segment of global input pixel (r, c): tile
    column c // 256 of input row r, in every octave that has that row, where the pair is fast."""
    _, W, _, _, kw = SHAPES[name]
    lr = r - kw.get("row_begin", 0)
    tc = c // TILE_COLS
    out = []
    for o, mask in enumerate(masks):
        seg = np.zeros_like(mask)
        if lr % (1 << o) == 0 and (lr >> o) < mask.shape[0]:
            c_lo = tc * TILE_COLS >> o
            seg[lr >> o, c_lo:min(c_lo + (TILE_COLS >> o), W >> o)] = True
        out.append(seg & mask)
    return out


def _top_levels(ctx, oracle, name, b):
    S = SHAPES[name][3]
    return [_bits(ctx.level(b, o, S + 2)) for o in range(_octaves(oracle, name))]


STORE_MAP = {  # shape, image, pixel row and column: in a fast tile, on a row every fused octave has
    "200x1028": ("200x1028", 0, 160, 16),
    "64x2048_o7": ("64x2048_o7", 0, 16, 1536),
    "96x768_b3": ("96x768_b3", 2, 32, 700),
    "band_hi": ("band_hi", 0, 576, 300),
    "odd_row": ("200x1028", 0, 37, 900),
}


@pytest.mark.parametrize("kern", KERNELS)
@pytest.mark.parametrize("case", sorted(STORE_MAP))
def test_poison_survives_exactly_on_the_rows_that_owe_no_store(pkg, oracle, case, kern):
    name, b, r, c = STORE_MAP[case]
    H, W, O, S, kw = SHAPES[name]
    L, Oo = S + 3, _octaves(oracle, name)
    P, Q = _nonneg(oracle, name)
    N = _with_pixel(Q, b, r, c, -1)
    B = len(P)
    with pkg.PyramidContext(H, W, S=S, octaves=O, **kw) as ctx:
        masks = _fast_masks(oracle, ctx, name)
        assert sum(int(m.sum()) for m in masks) > 0
        seg = _row_segment(masks, ctx, name, r, c)
        assert int(seg[0].sum()) > 0, "the pixel's tile stores octave 0 from registers"
        ctx.set_tuning(keep_kernel=kern)
        for imgs in (P, Q, P):
            _load(ctx, name, imgs)
            ctx.build()
        assert _known(ctx) == 1
        _poison(ctx)
        assert _known(ctx) == 1  # nobody told the library
        _load(ctx, name, Q)
        ctx.build()  # non-negative over a map of zeros: no fast pair stores anything
        ctx.sync()
        for i in range(B):
            want = _levels(oracle, name, ("Q", i), Q[i])
            for o, got in enumerate(_top_levels(ctx, oracle, name, i)):
                w = _bits(_cut(ctx, want, o, S + 2, L))
                fast = masks[o] if o < len(masks) else np.zeros(got.shape, bool)
                assert (got[fast] == POISON).all(), (case, kern, i, o, "a store that was not owed was made")
                assert (w[fast] == 0).all()  # what the builds before left there: +0
                _assert_bits(got[~fast], w[~fast], (case, kern, i, o, "slow pairs and tails store as ever"))
        _load(ctx, name, N)
        ctx.build()  # the pixel's row segment stores in every fused octave that has the row, nothing else does
        ctx.sync()
        for i in range(B):
            want = _levels(oracle, name, ("N", case) if i == b else ("Q", i), N[i])
            for o, got in enumerate(_top_levels(ctx, oracle, name, i)):
                w = _bits(_cut(ctx, want, o, S + 2, L))
                fast = masks[o] if o < len(masks) else np.zeros(got.shape, bool)
                stored = seg[o] if (i == b and o < len(masks)) else np.zeros(got.shape, bool)
                assert (got[fast & ~stored] == POISON).all(), (case, kern, i, o, "stored outside the pixel's row segment")
                _assert_bits(got[~fast | stored], w[~fast | stored], (case, kern, i, o, "the row segment"))
        assert sum(int(s.sum()) for s in seg) > 0
        # the restoring build stores the segment once more (+0 over the -0), the one after nothing
        _load(ctx, name, P)
        ctx.build()
        _poison(ctx)
        _load(ctx, name, Q)
        ctx.build()
        ctx.sync()
        for i in range(B):
            for o, got in enumerate(_top_levels(ctx, oracle, name, i)):
                if o < len(masks):
                    assert (got[masks[o]] == POISON).all(), (case, kern, i, o, "the flag was not cleared")


@pytest.mark.parametrize("kern", KERNELS)
def test_keep_signs_off_stores_all_of_level_s_plus_2(pkg, oracle, kern):
    name, b, r, c = STORE_MAP["200x1028"]
    H, W, O, S, kw = SHAPES[name]
    P, Q = _nonneg(oracle, name)
    N = _with_pixel(Q, b, r, c, -1)
    with pkg.PyramidContext(H, W, S=S, octaves=O, **kw) as ctx:
        ctx.set_tuning(keep_kernel=kern, keep_signs=0)
        assert ctx.tuning()["keep_signs"] == 0
        for imgs in (P, Q, P):
            _load(ctx, name, imgs)
            ctx.build()
            assert _known(ctx) == 0
        for imgs, key in ((Q, ("Q", 0)), (N, ("N", "200x1028"))):
            _poison(ctx)
            _load(ctx, name, imgs)
            ctx.build()
            ctx.sync()
            want = _levels(oracle, name, key, imgs[0])
            for o, got in enumerate(_top_levels(ctx, oracle, name, 0)):
                _assert_bits(got, _bits(_cut(ctx, want, o, S + 2, S + 3)), (kern, key, o))
            assert _known(ctx) == 0


# ---------------------------------------------------------------------------------------------
# GDP_TUNE_SIGNS_KNOWN against a model
# ---------------------------------------------------------------------------------------------
def test_signs_known_follows_the_model(pkg, oracle):
    name = "200x1028"
    H, W, O, S, kw = SHAPES[name]
    P, Q = _nonneg(oracle, name)

    def build(ctx, imgs=P):
        _load(ctx, name, imgs)
        ctx.build()

    with pkg.PyramidContext(H, W, S=S, octaves=O) as ctx:
        assert _known(ctx) == 0  # after create
        ctx.set_tuning(keep_kernel=1)
        build(ctx)
        assert _known(ctx) == 0  # the full build
        build(ctx)
        assert _known(ctx) == 1  # an int32 k_keep build
        ctx.set_tuning(keep_kernel=0)
        assert _known(ctx) == 1
        build(ctx)
        assert _known(ctx) == 0  # the build kernel's keep path does not keep the map
        ctx.set_tuning(keep_kernel=2)
        build(ctx)
        assert _known(ctx) == 1
        # readers and keep_kernel 1 <-> 2 leave it (the map is per row, whatever the rows per wave)
        ctx.level(0, 0, S + 2)
        ctx.pyramid(0)
        ctx.checksum(0)
        ctx.set_tuning(keep_kernel=1)
        assert _known(ctx) == 1
        build(ctx, Q)
        assert _known(ctx) == 1
        _check(ctx, oracle, name, [(("Q", 0), Q[0])], "after 2 -> 1")
        # every pyramid writer
        writers = {
            "pyramid_written": lambda: ctx.pyramid_written(0),
            "init": lambda: ctx.init(),
            "upload_level": lambda: ctx.upload_level(0, 1, 4, np.full(ctx.level_dims(1)[:2], np.nan, np.float32)),
            "upload_pyramid": lambda: ctx.upload_pyramid(np.full(ctx.packed_floats(), np.nan, np.float32)),
            "generate_dog": lambda: ctx.generate_dog(),
        }
        for what, write in writers.items():
            assert _known(ctx) == 1, what
            write()
            assert _known(ctx) == 0 and ctx.tuning()["zeros_clean"] == 0, what
            build(ctx)
            assert _known(ctx) == 0, what  # a full build
            build(ctx)
            assert _known(ctx) == 1, what
        # a switch of the knob, either way
        ctx.set_tuning(keep_signs=1)
        assert _known(ctx) == 1  # no switch
        ctx.set_tuning(keep_signs=0)
        assert _known(ctx) == 0 and ctx.tuning()["zeros_clean"] == 1
        build(ctx)
        assert _known(ctx) == 0
        ctx.set_tuning(keep_signs=1)
        assert _known(ctx) == 0
        build(ctx)
        assert _known(ctx) == 1
        with pytest.raises(pkg.GdpError):
            ctx.set_tuning(keep_signs=2)
        # a uint8 build
        ctx.set_input_format("u8")
        assert _known(ctx) == 1  # the input format is not the pyramid
        ctx.set_input((P[0] & 0xFF).astype(np.uint8))
        ctx.build()
        assert _known(ctx) == 0 and ctx.tuning()["zeros_clean"] == 1
        ctx.set_input_format("i32")
        build(ctx, Q)
        assert _known(ctx) == 1
        _check(ctx, oracle, name, [(("Q", 0), Q[0])], "after uint8")


@pytest.mark.parametrize("kern", KERNELS)
def test_input_format_switches_with_mostly_negative_images_stay_exact(pkg, oracle, kern):
    """int32 -> uint8 -> int32, the int32 images mostly negative: the uint8 build stores +0 over
    every -0 and leaves the map unknown, so the int32 build after it establishes it again; the
    build after that (non-negative) must restore every row that build left negative."""
    name = "200x1028"
    H, W, O, S, _ = SHAPES[name]
    rng = np.random.default_rng(78)
    neg = [-(rng.integers(1, 2**31 - 1, size=(H, W), dtype=np.int64)).astype(np.int32) for _ in range(2)]
    for n in neg:
        n[rng.integers(0, H, 300), rng.integers(0, W, 300)] = 5
        n[100:140] = np.abs(n[100:140])
    u8 = rng.integers(0, 256, size=(H, W), dtype=np.int64).astype(np.uint8)
    P, _ = _nonneg(oracle, name)
    steps = [("i32", P[0], ("P", 0)), ("i32", neg[0], ("neg", 0)), ("i32", neg[1], ("neg", 1)), ("u8", u8, ("u8", 0)),
             ("i32", neg[0], ("neg", 0)), ("i32", P[0], ("P", 0)), ("i32", P[0], ("P", 0))]
    with pkg.PyramidContext(H, W, S=S, octaves=O) as ctx:
        ctx.set_tuning(keep_kernel=kern)
        for k, (fmt, img, key) in enumerate(steps):
            ctx.set_input_format(fmt)
            ctx.set_input(img)
            ctx.build()
            assert _known(ctx) == (1 if fmt == "i32" and k > 0 else 0), k  # build 0 is the full build
            _check(ctx, oracle, name, [(key, img)], (kern, k))
