"""GDP_TUNE_KEEP_KERNEL: the steady-state build's own kernel (k_keep, csrc/gdp_keep.inc).

A build on a clean context-owned pyramid owes, outside the windows' support, only level S+2 =
copysign(0, x).  k_keep stores it for every fused octave from the registers that hold the octave-0
pixels, per (16 x 256 tile, octave) where the octave's footprint of the tile misses the support,
and sends every other (tile, octave), the tail octaves and ineligible contexts (W % 4 != 0, no
vector loads) through the build kernel's per-group keep path.

Every comparison is bitwise on uint32 views, every level of every octave, +-0 included, between
three builds of image B: the oracle's, a fresh context built once with keep_zeros = 0, and the
rebuild (after image A, whose signs are the opposite) of a clean context — with keep_kernel = 0
(the parent's kernel) and with every k_keep shape.  The shapes take each branch of the kernel
(clean tiles per octave computed on the CPU from the oracle's taps, 16 x 256 tiles):
  200 x 1028, O 5   W % 16 != 0 and H % 16 != 0 (both store masks); 55 / 49 / 39 / 39 / 17 of 65
                    tiles clean for octaves 0..4: every octave takes both paths
  64 x 2048, O 5    24 / 24 / 24 / 24 / 16 of 32 clean; the column support straddles the tile seam
  64 x 2048, O 7    the tail octaves 5 and 6
  512 x 512, O 5    octave 4 has no clean tile, octave 3 has 4 of 64
  96 x 768, O 3     batch 3 (image stride), with S = 0, 2 and 3 (level S+2 at a run-time L)
  203 x 331         W % 4 != 0: not eligible, the knob changes nothing
  1024 x 512        two row bands (row0 != 0)
  uint8 input       level S+2 is +0 everywhere outside the support
  bound device input with a pitch that is no multiple of 4: no vector loads, not eligible
The last tests name the paths that tests/test_gpu_steady_fuzz.py draws at random, so a regression
names itself without a seed: the grid-stride loop under a grid cap (tail units included), plain
stores (nontemporal = 0), the input format switched between kept builds, and the smallest shapes
with every octave count.
Runs on an MI355X.
"""
import numpy as np
import pytest
from steady_cases import _poison, _skipped, _support  # the store map of a kept build, shared with the sweep

pytestmark = pytest.mark.gpu

POISON = np.uint32(0xFFFFFFFF)
KERNELS = (1, 2)  # GDP_TUNE_KEEP_KERNEL values that select k_keep (4 / 2 rows per wave)
INT32_MIN = np.iinfo(np.int32).min


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _assert_same(got, want, what):
    g, w = _bits(got).ravel(), _bits(want).ravel()
    assert g.shape == w.shape, (what, g.shape, w.shape)
    bad = np.flatnonzero(g != w)
    assert bad.size == 0, f"{what}: {bad.size} words differ, first at {bad[:5]}: {g[bad[:5]]} vs {w[bad[:5]]}"


def _images(oracle, H, W, seed=12345):
    """(A, B): A positive on top, negative below, with zeros and INT32_MIN; B the opposite sign
    over large areas (so a stale sign shows), its own zeros and INT32_MIN."""
    a = oracle.lcg_image(H, W, seed)
    a[H // 2:] *= -1
    a[::7, ::5] = 0
    a[::11, ::13] = INT32_MIN
    b = -a  # INT32_MIN stays INT32_MIN
    rng = np.random.default_rng(H + W)
    b[rng.integers(0, H, 400), rng.integers(0, W, 400)] = 0
    b[rng.integers(0, H, 100), rng.integers(0, W, 100)] = INT32_MIN
    b[0, 0], b[-1, -1] = -1, -1  # corners far outside every support: sign bit only
    return a, b


def _want_levels(oracle, ctx, img, H, W, S, O):
    """The oracle's levels of `img` cut to the rows the (band) context holds, [o * L + s]."""
    lv = oracle.levels(oracle.build_pyramid(np.asarray(img, np.int32), S, O), H, W, S, O)
    out = []
    for o in range(O):
        rows, _, first = ctx.level_dims(o)
        out += [lv[(o, s)][first:first + rows] for s in range(S + 3)]
    return out


def _check_levels(ctx, b, want, S, O, what):
    for o in range(O):
        for s in range(S + 3):
            _assert_same(ctx.level(b, o, s), want[o * (S + 3) + s], (what, b, o, s))


# name: H, W, octaves (0 = all), S, context keywords
CASES = {
    "200x1028": (200, 1028, 5, 2, {}),
    "64x2048_o5": (64, 2048, 5, 2, {}),
    "64x2048_o7": (64, 2048, 7, 2, {}),
    "512x512": (512, 512, 5, 2, {}),
    "96x768_b3": (96, 768, 3, 2, dict(batch=3)),
    "96x768_b3_s0": (96, 768, 3, 0, dict(batch=3)),
    "96x768_b3_s3": (96, 768, 3, 3, dict(batch=3)),
    "203x331": (203, 331, 0, 2, {}),
    "band_lo": (1024, 512, 5, 2, dict(row_begin=0, row_end=512)),
    "band_hi": (1024, 512, 5, 2, dict(row_begin=512, row_end=1024)),
    "u8": (200, 1028, 5, 2, dict(input_format="u8")),
}


def _case_images(oracle, name):
    H, W, O, S, kw = CASES[name]
    if kw.get("input_format") == "u8":
        a = (oracle.lcg_image(H, W, 5) & 0xFF).astype(np.uint8)
        b = (255 - a).astype(np.uint8)
        b[::3, ::11] = 0
        return a, b
    return _images(oracle, H, W, 99 + H)


@pytest.mark.parametrize("name", sorted(CASES))
def test_rebuild_is_the_oracle_with_every_keep_kernel(pkg, oracle, name):
    H, W, O, S, kw = CASES[name]
    Oo = O or oracle.default_octaves(H, W)
    B = kw.get("batch", 1)
    r0, r1 = kw.get("row_begin", 0), kw.get("row_end", H)
    fmt = np.uint8 if kw.get("input_format") == "u8" else np.int32
    pair = _case_images(oracle, name)
    # image i of the batch in build k: alternate the pair so every image changes sign between builds
    seq = [[pair[(k + i) % 2] for i in range(B)] for k in range(2)]
    want = None
    # (keep_zeros, keep_kernel): the fresh full build, the parent's kept rebuild, k_keep's shapes
    for keep, kern in [(0, 0), (1, 0)] + [(1, k) for k in KERNELS]:
        with pkg.PyramidContext(H, W, S=S, octaves=O, **kw) as ctx:
            assert ctx.O == Oo
            if want is None:
                want = [_want_levels(oracle, ctx, seq[1][i], H, W, S, Oo) for i in range(B)]
            ctx.set_tuning(keep_zeros=keep, keep_kernel=kern)
            for k in range(2) if keep else (1,):  # keep_zeros = 0: one build of a fresh context
                for i in range(B):
                    ctx.set_input(np.ascontiguousarray(seq[k][i][r0:r1], dtype=fmt), i)
                ctx.build()
                assert ctx.tuning()["zeros_clean"] == 1
            ctx.sync()
            for i in range(B):
                _check_levels(ctx, i, want[i], S, Oo, (name, keep, kern))


def test_bound_input_without_vector_loads_is_not_taken(pkg, oracle):
    """A caller's device input whose pitch is no multiple of 4 allows no vector load (vec_in = 0):
    the context is not eligible and every knob value gives the oracle's bits; the same context
    with its own (aligned) input again runs k_keep."""
    import torch

    H, W, O, S, pitch = 96, 768, 3, 2, 771
    a, b = _images(oracle, H, W, 7)
    host = np.zeros((2, H, pitch), np.int32)
    host[0, :, :W], host[1, :, :W] = a, b
    dev = torch.from_numpy(host).cuda()
    for kern in (0,) + KERNELS:
        with pkg.PyramidContext(H, W, S=S, octaves=O) as ctx:
            ctx.set_tuning(keep_kernel=kern)
            want = _want_levels(oracle, ctx, b, H, W, S, O)
            for k in range(2):
                ctx.bind_device_input(dev[k].data_ptr(), pitch, H * pitch, keepalive=dev)
                ctx.build(torch.cuda.current_stream())
            torch.cuda.synchronize()
            _check_levels(ctx, 0, want, S, O, ("bound", kern))
            ctx.unbind_device_input()
            ctx.set_input(a)
            ctx.build()
            ctx.set_input(b)
            ctx.build()
            ctx.sync()
            _check_levels(ctx, 0, want, S, O, ("unbound", kern))


@pytest.mark.parametrize("name", ["200x1028", "band_hi"])
@pytest.mark.parametrize("kern", KERNELS)
def test_poison_survives_exactly_where_the_stores_are_skipped(pkg, oracle, name, kern):
    """After a build the pyramid is overwritten with 0xFF bytes behind the library's back; the
    k_keep rebuild leaves the poison exactly in the DoG levels outside the support and stores level
    S+2 and everything inside the support correctly — a store to a wrong level, row or octave shows
    as a missing poison word or as a wrong one."""
    H, W, O, S, kw = CASES[name]
    L = S + 3
    r0, r1 = kw.get("row_begin", 0), kw.get("row_end", H)
    a, b = _case_images(oracle, name)
    with pkg.PyramidContext(H, W, S=S, octaves=O, **kw) as ctx:
        skipped = _skipped(oracle, H, W, O, S, [ctx.level_dims(o) for o in range(O)])
        ctx.set_tuning(keep_kernel=kern)
        ctx.set_input(a[r0:r1])
        ctx.build()
        _poison(ctx)
        assert ctx.tuning()["zeros_clean"] == 1  # nobody told the library
        ctx.set_input(b[r0:r1])
        ctx.build()
        ctx.sync()
        want = _want_levels(oracle, ctx, b, H, W, S, O)
        n_poison = 0
        for o in range(O):
            sk = skipped[o]
            for s in range(L):
                got, w = _bits(ctx.level(0, o, s)), _bits(want[o * L + s])
                if s < L - 1:
                    assert sk.shape == got.shape, (o, sk.shape, got.shape)
                    assert (got[sk] == POISON).all(), ("a skipped store was made", o, s)
                    assert (w[sk] == 0).all()  # what the earlier build left there: +0
                    _assert_same(got[~sk], w[~sk], ("inside the support", o, s))
                    n_poison += int(sk.sum())
                else:
                    _assert_same(got, w, ("level S+2", o))
        assert n_poison > 0
        ctx.pyramid_written(-1)
        ctx.build()
        ctx.sync()
        _check_levels(ctx, 0, want, S, O, "after pyramid_written")


def test_knob_round_trip(pkg, oracle):
    """set_tuning(keep_kernel=) reads back, refuses values that name no kernel, and is a launch-time
    choice: switching it between builds neither clears nor sets GDP_TUNE_ZEROS_CLEAN."""
    H, W, O, S, _ = CASES["200x1028"]
    a, b = _case_images(oracle, "200x1028")
    with pkg.PyramidContext(H, W, S=S, octaves=O) as ctx:
        default = ctx.tuning()["keep_kernel"]
        assert default in (0,) + KERNELS
        for v in (0,) + KERNELS:
            ctx.set_tuning(keep_kernel=v)
            assert ctx.tuning()["keep_kernel"] == v
            assert ctx.tuning()["zeros_clean"] == 0
        for bad in (-1, len(KERNELS) + 1, 1 << 20):
            with pytest.raises(pkg.GdpError):
                ctx.set_tuning(keep_kernel=bad)
            assert ctx.tuning()["keep_kernel"] == KERNELS[-1]
        ctx.set_input(a)
        ctx.build()
        want = _want_levels(oracle, ctx, b, H, W, S, O)
        ctx.set_input(b)
        for v in (0,) + KERNELS + (0, 1):
            ctx.set_tuning(keep_kernel=v)
            assert ctx.tuning()["zeros_clean"] == 1
            ctx.build()
            assert ctx.tuning()["zeros_clean"] == 1
        ctx.sync()
        _check_levels(ctx, 0, want, S, O, "after switching")
        assert ctx.tuning()["keep_zeros"] == 1


MUTATORS = {
    "first_build": None,
    "pyramid_written": lambda c: c.pyramid_written(0),
    "init": lambda c: c.init(),
    "upload_level": lambda c: c.upload_level(0, 1, 4, np.full(c.level_dims(1)[:2], np.nan, np.float32)),
}


@pytest.mark.parametrize("name", sorted(MUTATORS))
@pytest.mark.parametrize("kern", KERNELS)
def test_a_context_with_the_keep_kernel_still_stores_every_byte_when_it_must(pkg, oracle, name, kern):
    """keep_kernel >= 1 changes only the build of a CLEAN pyramid: the first build of a context and
    the build after a mutator overwrite every byte of a poisoned pyramid."""
    H, W, O, S, _ = CASES["200x1028"]
    a, b = _case_images(oracle, "200x1028")
    with pkg.PyramidContext(H, W, S=S, octaves=O) as ctx:
        ctx.set_tuning(keep_kernel=kern)
        if MUTATORS[name] is not None:
            ctx.set_input(a)
            ctx.build()
            assert ctx.tuning()["zeros_clean"] == 1
            MUTATORS[name](ctx)
        assert ctx.tuning()["zeros_clean"] == 0
        _poison(ctx)
        ctx.set_input(b)
        ctx.build()
        ctx.sync()
        _check_levels(ctx, 0, _want_levels(oracle, ctx, b, H, W, S, O), S, O, (name, kern))
        assert ctx.tuning()["zeros_clean"] == 1


def test_time_builds_and_autotune_leave_a_correct_pyramid(pkg, oracle):
    """The build timers run k_keep for their timed launches; both leave the oracle's bits."""
    H, W, O, S, _ = CASES["64x2048_o7"]
    _, b = _case_images(oracle, "64x2048_o7")
    with pkg.PyramidContext(H, W, S=S, octaves=O) as ctx:
        want = _want_levels(oracle, ctx, b, H, W, S, O)
        ctx.set_input(b)
        ctx.upload_pyramid(np.full(ctx.packed_floats(), np.nan, np.float32))
        assert ctx.time_builds(2) > 0
        _check_levels(ctx, 0, want, S, O, "time_builds")
        ctx.upload_pyramid(np.full(ctx.packed_floats(), np.nan, np.float32))
        ctx.autotune(iters=1)
        _check_levels(ctx, 0, want, S, O, "autotune")


# ---- fixed-name cases of the paths the steady-state sweep (test_gpu_steady_fuzz.py) draws at random --
_WANTS = {}  # (name, image of the batch) -> the oracle's levels of the rebuild's image: computed once, never modified


def _kept_rebuild(pkg, oracle, name, what, **tuning):
    """Image A, then image B on the same (clean) context under `tuning`; the kept rebuild must be
    the oracle's build of B in every level of every image."""
    H, W, O, S, kw = CASES[name]
    B = kw.get("batch", 1)
    pair = _case_images(oracle, name)
    seq = [[pair[(k + i) % 2] for i in range(B)] for k in range(2)]
    with pkg.PyramidContext(H, W, S=S, octaves=O, **kw) as ctx:
        ctx.set_tuning(**tuning)
        for k in range(2):
            for i in range(B):
                ctx.set_input(seq[k][i], i)
            assert ctx.tuning()["zeros_clean"] == k
            ctx.build()
        assert ctx.tuning()["zeros_clean"] == 1
        ctx.sync()
        for i in range(B):
            if (name, i) not in _WANTS:
                _WANTS[(name, i)] = _want_levels(oracle, ctx, seq[1][i], H, W, S, O)
            _check_levels(ctx, i, _WANTS[(name, i)], S, O, (name, what, tuning))


GRID_CASES = ("200x1028", "64x2048_o7", "96x768_b3")
# 200x1028: 65 tiles; 64x2048_o7: 32 tiles and the tail units of octaves 5 and 6; 96x768_b3: 54 tiles of 3 images
GRID_CAPS = {"grid1": dict(grid=1), "grid3": dict(grid=3), "blocks_per_cu1": dict(blocks_per_cu=1)}


@pytest.mark.parametrize("cap", sorted(GRID_CAPS))
@pytest.mark.parametrize("kern", KERNELS)
@pytest.mark.parametrize("name", GRID_CASES)
def test_grid_capped_keep_kernel_rebuild_is_the_oracle(pkg, oracle, name, kern, cap):
    """k_keep's grid-stride loop: with GDP_TUNE_GRID = 1 / 3 one block walks every unit (a third of
    them), tiles of every image and — 64x2048_o7 — the tail units after them; blocks_per_cu = 1 caps
    the grid at one block per CU."""
    _kept_rebuild(pkg, oracle, name, cap, keep_kernel=kern, **GRID_CAPS[cap])


@pytest.mark.parametrize("kern", KERNELS)
@pytest.mark.parametrize("name", GRID_CASES)
def test_keep_kernel_with_plain_stores_is_the_oracle(pkg, oracle, name, kern):
    """nontemporal = 0 launches k_keep<false, *>: the same bits through plain stores."""
    _kept_rebuild(pkg, oracle, name, "nontemporal=0", keep_kernel=kern, nontemporal=0)
    _kept_rebuild(pkg, oracle, name, "nontemporal=0, grid=3", keep_kernel=kern, nontemporal=0, grid=3)


@pytest.mark.parametrize("kern", (0,) + KERNELS)
def test_input_format_switches_between_kept_builds(pkg, oracle, kern):
    """int32 -> uint8 -> int32 across three kept builds, the int32 images mostly negative: the
    uint8 build owes +0 in all of level S+2 outside the support (inside it the level is the last
    Gaussian of pixels >= 0: no sign bit anywhere) — it must overwrite the -0 the int32 build left,
    a kernel that stored nothing for uint8 input would leave them — and the int32 build after it
    the oracle's signs again."""
    H, W, O, S, _ = CASES["200x1028"]
    first, _ = _case_images(oracle, "200x1028")
    rng = np.random.default_rng(77)
    neg = [-(rng.integers(1, 2**31 - 1, size=(H, W), dtype=np.int64)).astype(np.int32) for _ in range(2)]
    for n in neg:
        n[rng.integers(0, H, 300), rng.integers(0, W, 300)] = 0
        n[rng.integers(0, H, 300), rng.integers(0, W, 300)] = 5
        n[rng.integers(0, H, 100), rng.integers(0, W, 100)] = INT32_MIN
    u8 = rng.integers(0, 256, size=(H, W), dtype=np.int64).astype(np.uint8)
    support = _support(oracle, H, W, O, S)
    with pkg.PyramidContext(H, W, S=S, octaves=O) as ctx:
        ctx.set_tuning(keep_kernel=kern)
        ctx.set_input(first)
        ctx.build()
        for step, (fmt, img) in enumerate([("i32", neg[0]), ("u8", u8), ("i32", neg[1])]):
            ctx.set_input_format(fmt)
            assert ctx.tuning()["zeros_clean"] == 1, (step, "the input format is not the pyramid")
            ctx.set_input(img)
            ctx.build()
            assert ctx.tuning()["zeros_clean"] == 1
            ctx.sync()
            want = _want_levels(oracle, ctx, img, H, W, S, O)
            for o in range(O):
                top, w = _bits(ctx.level(0, o, S + 2)), _bits(want[o * (S + 3) + S + 2])
                if fmt == "u8":
                    rows, cols = support[o]
                    outside = ~(rows[:, None] & cols[None, :])
                    assert outside.mean() > 0.5 or o >= 3
                    assert not top[outside].any(), (step, o, "level S+2 of a uint8 build is +0 outside the support",
                                                    int(np.count_nonzero(top[outside])))
                    assert not (top & 0x80000000).any(), (step, o, "a uint8 build left a sign bit in level S+2")
                else:
                    assert (w == 0x80000000).mean() > 0.5  # the image does what the test needs: mostly -0
                    _assert_same(top, w, (step, o, "the oracle's signs"))
            _check_levels(ctx, 0, want, S, O, ("format", kern, step))


# the smallest shapes: one group, one tile column of one group, a second tile column of one group
# (17 x 260: every lane but one clamped and masked), less than one tile row
SMALL = {"1x4": (1, 4), "16x4": (16, 4), "17x260": (17, 260), "15x512": (15, 512)}


@pytest.mark.parametrize("octaves", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("kern", KERNELS)
@pytest.mark.parametrize("shape", sorted(SMALL))
def test_smallest_shapes_with_every_octave_count(pkg, oracle, shape, kern, octaves):
    """Octaves forced to 1..4 (kp_F < 5: oct[o] beyond O holds no rows) and the default; an octave
    count the shape does not have is refused at creation."""
    H, W = SMALL[shape]
    S = 2
    if octaves > oracle.default_octaves(H, W):
        with pytest.raises(pkg.GdpError):
            pkg.PyramidContext(H, W, S=S, octaves=octaves)
        return
    O = octaves or oracle.default_octaves(H, W)
    a, b = _images(oracle, H, W, 31 + H)
    c = -b
    with pkg.PyramidContext(H, W, S=S, octaves=octaves) as ctx:
        assert ctx.O == O
        ctx.set_tuning(keep_kernel=kern)
        for k, img in enumerate((a, b, c)):
            ctx.set_input(img)
            assert ctx.tuning()["zeros_clean"] == min(k, 1)
            ctx.build()
            ctx.sync()
            _check_levels(ctx, 0, _want_levels(oracle, ctx, img, H, W, S, O), S, O, (shape, kern, octaves, k))
