"""Shared by the steady-state sweep (a plain module, no fixtures, no GPU): the generator of random
build SEQUENCES on one context, the model of GDP_TUNE_ZEROS_CLEAN they carry, and the store map of a
kept build.  tests/test_steady_cases.py checks on the CPU that the default seed reaches the hard
paths; tests/test_gpu_steady_fuzz.py runs the cases on an MI355X.

A case is a plain dict (draw): a geometry, the build knobs, three builds with three different images
(image k+1 has the opposite sign of image k over large areas, each its own zeros and INT32_MIN
pixels: a store that is owed but skipped, or made from the wrong pixel, changes bits), and one event
before build 2 and one before build 3.  case["builds"][k] is the model's state when build k is
launched — "clean" the expected GDP_TUNE_ZEROS_CLEAN, "k_keep" whether the steady-state kernel
(csrc/gdp_keep.inc) takes it; every event carries "clean", the flag the model expects after it.
"""
import ctypes

import numpy as np
from conftest import BUILD_VARIANTS

INT32_MIN = np.iinfo(np.int32).min
POISON = np.uint32(0xFFFFFFFF)
TILE_ROWS, TILE_COLS, FUSED, TAIL_GROUPS = 16, 256, 5, 256  # k_keep's units (csrc/gdp_geom.inc)
KNOBS = ("variant", "tile_order", "zero_window", "nontemporal", "keep_kernel", "grid", "blocks_per_cu")
EVENT_KINDS = ("none", "reader", "refine", "knob", "format", "bind_in", "unbind_in", "mutator", "centre", "bind_out",
               "unbind_out", "poison")
READERS = ("level", "pyramid", "detect_extrema", "keypoints")
MUTATORS = ("upload_level", "generate_dog", "gauss_range", "init", "pyramid_written")
N_BUILDS = 3
DEFAULT_SEED, DEFAULT_CASES, CHUNK = 20261020, 160, 40  # the suite's sweep: four chunks of 40 cases


# ---------------------------------------------------------------------------------------------
# the store map of a kept build
# ---------------------------------------------------------------------------------------------
def _support(oracle, H, W, O, S):
    """Per octave: (rows, cols) boolean masks of the window support — some tap of some scale,
    under either window centre, is non-zero."""
    out = []
    for o in range(O):
        masks = []
        for n in (H, W):
            m = np.zeros(n >> o, bool)
            for centre in ("serial", "intlen"):
                for s in range(S + 3):
                    t = oracle.taps(n, o, s, centre)[:n >> o]
                    m[:t.size] |= t != 0
            masks.append(m)
        out.append(tuple(masks))
    return out


def _skipped(oracle, H, W, O, S, dims=None):
    """Per octave, the pixels whose DoG stores a kept build skips: rows outside the row support,
    and 4-pixel groups wholly outside the column support.  `dims`: the context's level_dims per
    octave (rows held, cols, first global row); None = the whole image."""
    out = []
    for o, (rows, cols) in enumerate(_support(oracle, H, W, O, S)):
        n = cols.size
        grp = np.zeros(n, bool)
        for c in range(0, n, 4):
            grp[c:c + 4] = not cols[c:c + 4].any()
        nrows, _, first = dims[o] if dims else (H >> o, n, 0)
        out.append(~rows[first:first + nrows, None] | grp[None, :])
    return out


def _poison(ctx):
    """0xFF over the whole context-owned pyramid, behind the library's back."""
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemset.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t]
    hip.hipDeviceSynchronize.argtypes = []
    ctx.sync()
    assert hip.hipMemset(ctypes.c_void_p(ctx.device_level_ptr(0, 0, 0)), 0xFF, ctx.pyramid_bytes()) == 0
    assert hip.hipDeviceSynchronize() == 0


def skipped_fraction(oracle, case):
    """The share of the whole image's DoG words (levels 0..S+1) that a kept build does not store."""
    sk = _skipped(oracle, case["H"], case["W"], case["Oeff"], case["S"])
    total = sum(m.size for m in sk)
    return sum(int(m.sum()) for m in sk) / total if total else 0.0


def band_dims(case, span):
    """level_dims of the context that holds input rows [span): per octave (rows, cols, first row).
    The cuts are multiples of 2^(max(O, 5) - 1), so every octave's rows split exactly."""
    r0, r1 = span
    return [((r1 >> o) - (r0 >> o), case["W"] >> o, r0 >> o) for o in range(case["Oeff"])]


def spans(case):
    return case["bands"] or [(0, case["H"])]


def keep_units(case):
    """Work units of one k_keep launch of the case's smallest context: its 16 x 256 tiles and the
    256-group slices of the octaves beyond the fused ones."""
    W, B = case["W"], case["B"]
    span = min(spans(case), key=lambda s: s[1] - s[0])
    tiles = -(-(span[1] - span[0]) // TILE_ROWS) * -(-W // TILE_COLS) * B
    tail = sum(n * -(-c // 4) for n, c, _ in band_dims(case, span)[FUSED:])
    return tiles + -(-tail * B // TAIL_GROUPS)


def clean_tiles(oracle, case):
    """Per fused octave, the number of (tile, octave) pairs of one image that k_keep stores from
    registers: the octave's footprint of the 16 x 256 input tile misses the support's bounding
    ranges (its hit test, restated)."""
    H, W, O, S = case["H"], case["W"], case["Oeff"], case["S"]
    sup = _support(oracle, H, W, O, S)
    out = []
    for o in range(min(O, FUSED)):
        box = []
        for m in sup[o]:
            nz = np.flatnonzero(m)
            box.append((int(nz[0]), int(nz[-1]) + 1) if nz.size else (0, 0))
        (sr0, sr1), (sc0, sc1) = box
        n = 0
        for r0, r1 in spans(case):
            for tr in range(-(-(r1 - r0) // TILE_ROWS)):
                for tc in range(-(-W // TILE_COLS)):
                    r_lo = (r0 >> o) + (tr * TILE_ROWS >> o)
                    r_hi = r_lo + (TILE_ROWS >> o)
                    c_lo = tc * TILE_COLS >> o
                    c_hi = min(c_lo + (TILE_COLS >> o), W >> o)
                    n += not (r_lo < sr1 and r_hi > sr0 and c_lo < sc1 and c_hi > sc0)
        out.append(n)
    return out


# ---------------------------------------------------------------------------------------------
# the draw
# ---------------------------------------------------------------------------------------------
def _grid_cap(rng):
    """A grid cap: (grid, blocks_per_cu)."""
    g = int(rng.choice((1, 3, 7, 0)))
    return (g, 0) if g else (0, 1)


def _snapshot(state, W):
    st = dict(state)
    vec_in = not st["in_bound"] or st["pitch"] % 4 == 0
    st["eligible"] = W % 4 == 0 and vec_in
    st["kept"] = st["clean"] == 1  # keep_zeros stays 1; clean is never 1 while an output is bound
    st["k_keep"] = st["kept"] and st["keep_kernel"] > 0 and st["eligible"]
    return st


def _event(rng, case, state):
    """One event; updates the model `state` and returns the event with the flag expected after it."""
    whole = case["bands"] is None
    r = rng.random()
    if state["out_bound"] and r < 0.7:
        ev = dict(kind="unbind_out")
    elif state["in_bound"] and r < 0.3:
        ev = dict(kind="unbind_in")
    else:
        kind = str(rng.choice(("none", "reader", "refine", "knob", "format", "bind_in", "mutator", "centre", "bind_out", "poison"),
                              p=(0.06, 0.10, 0.12, 0.13, 0.13, 0.07, 0.11, 0.06, 0.10, 0.12)))
        if kind == "refine" and not whole:
            kind = "reader"
        if kind == "bind_in" and (not whole or state["in_bound"]):
            kind = "knob"
        if kind == "bind_out" and state["out_bound"]:
            kind = "format"
        if kind == "poison" and state["out_bound"]:
            kind = "none"  # only on an own pyramid whose build left the flag at 1
        ev = dict(kind=kind)
    kind = ev["kind"]
    if kind == "reader":
        ev["what"] = str(rng.choice(READERS if whole else READERS[:2]))
    elif kind == "refine":
        ev["contrast"], ev["edge_ratio"] = (0.0, 0.0) if rng.random() < 0.5 else (0.0, 10.0)
    elif kind == "knob":
        what = str(rng.choice(("variant", "zero_window", "keep_kernel", "grid")))
        ev["what"] = what
        if what == "variant":
            ev["set"] = dict(variant=int(rng.choice([v for v in BUILD_VARIANTS if v != state["variant"]])))
        elif what == "zero_window":
            ev["set"] = dict(zero_window=1 - state["zero_window"])
        elif what == "keep_kernel":
            ev["set"] = dict(keep_kernel=int(rng.choice([v for v in (0, 1, 2) if v != state["keep_kernel"]])))
        else:
            g, bpc = _grid_cap(rng)
            ev["set"] = dict(grid=g, blocks_per_cu=bpc)
        state.update(ev["set"])
    elif kind == "format":
        state["fmt"] = "u8" if state["fmt"] == "i32" else "i32"
        state["in_bound"] = False  # gdp_set_input_format gives the context a fresh input buffer of its own
        ev["fmt"] = state["fmt"]
    elif kind == "bind_in":
        state["in_bound"] = True
        state["pitch"] = case["W"] + int(rng.integers(0, 9))
        ev["pitch"] = state["pitch"]
    elif kind == "unbind_in":
        state["in_bound"] = False
    elif kind == "mutator":
        ev["what"] = str(rng.choice(MUTATORS if whole else ("upload_level", "pyramid_written")))
        ev["o"] = int(rng.integers(0, case["Oeff"]))
        ev["s"] = int(rng.integers(0, case["S"] + 3))
        ev["b"] = int(rng.integers(0, case["B"]))
        state["clean"] = 0
    elif kind == "centre":
        state["centre"] = "intlen" if state["centre"] == "serial" else "serial"
        ev["centre"] = state["centre"]
        state["clean"] = 0
    elif kind == "bind_out":
        state["out_bound"] = True
        state["clean"] = 0
    elif kind == "unbind_out":
        state["out_bound"] = False
        state["clean"] = 0
    ev["clean"] = state["clean"]
    return ev


def draw(rng):
    """One case from `rng` (a numpy Generator): pure, no GPU, no oracle."""
    if rng.random() < 0.15:  # wide and short: octaves 3 and 4 have clean tiles only where W >> o is well above 60
        H = int(rng.integers(1, 65))
        W = 4 * int(rng.integers(256, 526))
    else:
        H = int(rng.integers(1, 321))
        W = int(rng.integers(1, 641))
        if rng.random() < 0.6:
            W = -(-W // 4) * 4  # the k_keep-eligible widths
    r = rng.random()
    if r < 0.08:
        W = max(1, round(W / TILE_COLS)) * TILE_COLS + 4  # a last tile column of one 4-pixel group
    elif r < 0.16:
        H = int(rng.integers(1, TILE_ROWS))  # less than one tile row
    S = int(rng.integers(0, 5))
    omax = max(1, int(np.floor(np.log2(min(H, W)))) + 1)
    O = 0 if rng.random() < 0.5 else int(rng.integers(1, omax + 1))
    Oeff = O or omax
    B = int(rng.integers(1, 4))
    fmt = "u8" if rng.random() < 0.3 else "i32"
    device_input = bool(rng.random() < 0.3)
    pitch = W + int(rng.integers(0, 9))
    bands = None
    if rng.random() < 0.2:  # a row-band split: one image, host uploads, the alignment rule of test_gpu_fuzz.py's _case
        B, device_input = 1, False
        align = 1 << (max(Oeff, 5) - 1)
        cuts = sorted({0, H} | {c for c in range(align, H, align) if rng.random() < 0.5})
        if len(cuts) > 2:
            bands = [(a, b) for a, b in zip(cuts[:-1], cuts[1:])]
    grid, bpc = _grid_cap(rng) if rng.random() < 0.3 else (0, 0)
    knobs = dict(variant=int(rng.choice(BUILD_VARIANTS)), tile_order=int(rng.integers(0, 3)),
                 zero_window=int(rng.integers(0, 2)), nontemporal=int(rng.integers(0, 2)),
                 keep_kernel=int(rng.integers(0, 3)), grid=grid, blocks_per_cu=bpc)
    centre = "intlen" if rng.random() < 0.3 else "serial"
    case = dict(H=H, W=W, S=S, O=O, Oeff=Oeff, B=B, bands=bands, img_seed=int(rng.integers(0, 2**31)))
    state = dict(fmt=fmt, in_bound=device_input, pitch=pitch, out_bound=False, centre=centre, clean=0, **knobs)
    builds, events = [_snapshot(state, W)], []
    for _ in range(1, N_BUILDS):
        state["clean"] = 0 if state["out_bound"] else 1  # what a build leaves
        events.append(_event(rng, case, state))
        builds.append(_snapshot(state, W))
    case["builds"], case["events"] = builds, events
    return case


def cases(seed, n):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        c = draw(rng)
        c["id"] = i
        out.append(c)
    return out


def images(case):
    """[build][image]: the inputs of every build, in that build's input format."""
    H, W, B = case["H"], case["W"], case["B"]
    rng = np.random.default_rng(case["img_seed"])
    hi = 2**31 - 1 if rng.random() < 0.3 else 256  # the whole int32 range now and then
    split = int(rng.integers(0, H + 1))
    n = max(1, H * W // 40)
    out = []
    for k, st in enumerate(case["builds"]):
        per = []
        for b in range(B):
            mag = rng.integers(1, hi, size=(H, W), dtype=np.int64)
            if st["fmt"] == "u8":
                img = (mag & 0xFF).astype(np.uint8)
                if (k + b) % 2:
                    img = (255 - img).astype(np.uint8)
                img[rng.integers(0, H, n), rng.integers(0, W, n)] = 0
            else:
                img = mag.astype(np.int32)
                img[split:] *= -1
                if (k + b) % 2:  # the opposite sign of the build before, over large areas
                    img = -img
                img[rng.integers(0, H, n), rng.integers(0, W, n)] = 0
                img[rng.integers(0, H, max(1, n // 4)), rng.integers(0, W, max(1, n // 4))] = INT32_MIN
                if k % 2:
                    img[0, 0], img[-1, -1] = -1, -1  # corners far outside every support: sign bit only
            per.append(img)
        out.append(per)
    return out


def oracle_pyramids(oracle, case, imgs=None):
    """[build][image]: the oracle's packed pyramid of every input under that build's centre."""
    imgs = images(case) if imgs is None else imgs
    return [[oracle.build_pyramid(im.astype(np.int32), case["S"], case["Oeff"], centre=st["centre"]) for im in per]
            for per, st in zip(imgs, case["builds"])]
