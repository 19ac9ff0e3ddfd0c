"""Shared by the sign-map sweep (a plain module, no fixtures, no GPU): the CPU model of k_keep's sign
map (GDP_TUNE_KEEP_SIGNS, csrc/gdp_keep.inc), a generator of build sequences on which the map
matters, and the model run over the existing steady-state sweep (tests/steady_cases.py).
tests/test_keep_signs_cases.py checks on the CPU that the default seed reaches every path of the
rule; tests/test_gpu_keep_signs_fuzz.py runs the cases on an MI355X.

The rule: an int32 k_keep launch (`st["k_keep"]` and int32 input) runs mode 2 ("use") when the map
is known, else mode 1 ("establish"), and leaves it known; every other build leaves it unknown, and
so does every event that clears GDP_TUNE_ZEROS_CLEAN.  In mode 2 the row segment (image, band-local
input row, 256-column tile) runs its stores iff its flag is set or one of its pixels is negative;
either mode leaves flag = "a pixel of the segment is negative".
"""
import numpy as np
import steady_cases as sc

INT32_MIN = np.iinfo(np.int32).min
N_BUILDS = 5
# the suite's sweep: eight chunks of 40 cases.  Seed and count chosen so that the model alone reaches every path of
# the rule five times (tests/test_keep_signs_cases.py); the rarest is an establishing build after a keep_kernel = 0 build
DEFAULT_SEED, DEFAULT_CASES, CHUNK = 20261025, 320, 40
INVALIDATIONS = ("first", "mutator", "centre", "output", "poison", "uint8 build", "keep_kernel 0 build", "ineligible build")


def negatives(img_band, W):
    """[band-local row, tile column]: some pixel of the segment is negative (int32 input)."""
    tiles_c = -(-W // sc.TILE_COLS)
    pad = np.zeros((img_band.shape[0], tiles_c * sc.TILE_COLS), bool)
    pad[:, :W] = img_band < 0
    return pad.reshape(img_band.shape[0], tiles_c, sc.TILE_COLS).any(axis=2)


class SignMap:
    """The model of one context's map: `known` (GDP_TUNE_SIGNS_KNOWN) and the flags."""

    def __init__(self, rows, W, B):
        self.rows, self.W, self.B = rows, W, B
        self.known = False
        self.flags = np.zeros((B, rows, -(-W // sc.TILE_COLS)), bool)

    def invalidate(self):
        self.known = False

    def build(self, st, imgs_band):
        """One build in the state `st` (a steady_cases snapshot) of the band's images.  Returns
        (mode, stored, neg): stored[b, row, tile column] — the segment runs its register stores —
        and neg, the flags the launch leaves (both None in mode 0: not an int32 k_keep launch, every
        word of level S+2 is stored)."""
        if not (st["k_keep"] and st["fmt"] == "i32"):
            self.known = False
            return 0, None, None
        neg = np.stack([negatives(im, self.W) for im in imgs_band])
        if self.known:
            mode, stored = 2, self.flags | neg
        else:
            mode, stored = 1, np.ones_like(neg)
        self.flags, self.known = neg, True
        return mode, stored, neg


def fast_masks(oracle, case, span, dims):
    """Per fused octave, the words of level S+2 of the band that k_keep stores from registers (the
    hit test of steady_cases.clean_tiles, restated per word)."""
    H, W, O, S = case["H"], case["W"], case["Oeff"], case["S"]
    r0, r1 = span
    out = []
    for o, sup in enumerate(sc._support(oracle, H, W, O, S)[:sc.FUSED]):
        box = []
        for m in sup:
            nz = np.flatnonzero(m)
            box.append((int(nz[0]), int(nz[-1]) + 1) if nz.size else (0, 0))
        (sr0, sr1), (sc0, sc1) = box
        rows, cols, first = dims[o]
        mask = np.zeros((rows, cols), bool)
        for tr in range(-(-(r1 - r0) // sc.TILE_ROWS)):
            for tc in range(-(-W // sc.TILE_COLS)):
                l_lo = tr * sc.TILE_ROWS >> o
                r_lo, r_hi = first + l_lo, first + l_lo + (sc.TILE_ROWS >> o)
                c_lo = tc * sc.TILE_COLS >> o
                c_hi = min(c_lo + (sc.TILE_COLS >> o), W >> o)
                if not (r_lo < sr1 and r_hi > sr0 and c_lo < sc1 and c_hi > sc0):
                    mask[l_lo:l_lo + (sc.TILE_ROWS >> o), c_lo:c_hi] = True
        out.append(mask)
    return out


def unstored(masks, stored, b, dims):
    """Per fused octave, the words of level S+2 of image b that a mode-2 build leaves alone: in a
    fast pair, sourced from a segment that ran no stores."""
    out = []
    for o, mask in enumerate(masks):
        rows, cols, _ = dims[o]
        src_r = np.arange(rows) << o
        src_tc = (np.arange(cols) << o) // sc.TILE_COLS
        out.append(mask & ~stored[b][src_r[:, None], src_tc[None, :]])
    return out


# ---------------------------------------------------------------------------------------------
# the draw: steady_cases.draw's case, continued to five builds
# ---------------------------------------------------------------------------------------------
def _runnable(case):
    """The steady-state model takes every `upload_level` for a pyramid writer, but the upload of a
    level of which a row band holds no row (a coarse octave of a short last band) is no call at
    all: such a case is drawn again."""
    for ev in case["events"]:
        if ev["kind"] == "mutator" and ev["what"] == "upload_level" and case["bands"]:
            if any(sc.band_dims(case, span)[ev["o"]][0] == 0 for span in case["bands"]):
                return False
    return True


def draw(rng):
    case = _draw(rng)
    while not _runnable(case):
        case = _draw(rng)
    return case


def _draw(rng):
    case = sc.draw(rng)
    W = case["W"]
    state = {k: v for k, v in case["builds"][-1].items() if k not in ("eligible", "kept", "k_keep")}
    for _ in range(sc.N_BUILDS, N_BUILDS):
        state["clean"] = 0 if state["out_bound"] else 1  # what a build leaves
        case["events"].append(sc._event(rng, case, state))
        case["builds"].append(sc._snapshot(state, W))
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
    """[build][image]: per build and tile row non-negative with probability 0.6, else a few
    negative pixels in the tile row; now and then the whole int32 range with large negative areas;
    zeros and INT32_MIN as in steady_cases.images."""
    H, W, B = case["H"], case["W"], case["B"]
    rng = np.random.default_rng(case["img_seed"])
    n = max(1, H * W // 40)
    out = []
    for st in case["builds"]:
        per = []
        for _ in range(B):
            whole = rng.random() < 0.1
            mag = rng.integers(1, 2**31 - 1 if whole else 256, size=(H, W), dtype=np.int64)
            if st["fmt"] == "u8":
                img = (mag & 0xFF).astype(np.uint8)
                img[rng.integers(0, H, n), rng.integers(0, W, n)] = 0
            else:
                img = mag.astype(np.int32)
                img[rng.integers(0, H, n), rng.integers(0, W, n)] = 0
                if whole:
                    img[int(rng.integers(0, H + 1)):] *= -1
                    img[rng.integers(0, H, max(1, n // 4)), rng.integers(0, W, max(1, n // 4))] = INT32_MIN
                else:
                    for t0 in range(0, H, sc.TILE_ROWS):
                        if rng.random() < 0.6:
                            continue
                        k = int(rng.integers(1, 4))
                        rr = rng.integers(t0, min(t0 + sc.TILE_ROWS, H), k)
                        img[rr, rng.integers(0, W, k)] = rng.choice((-1, -255, INT32_MIN), k)
            per.append(img)
        out.append(per)
    return out


# ---------------------------------------------------------------------------------------------
# the model over a case: what every build does, and why
# ---------------------------------------------------------------------------------------------
def walk(case, imgs, poison_rebuild=True):
    """The model over the case's sequence as the sweeps run it (a poison event is followed by the
    store-map check, gdp_pyramid_written and a full rebuild).  Yields per build and band:
    dict(k, span, mode, stored, neg, old, after — the kind of invalidation an establishing build
    follows, or None —, poisoned — the build follows a poison event)."""
    spans = sc.spans(case)
    maps = [SignMap(r1 - r0, case["W"], case["B"]) for r0, r1 in spans]
    why = ["first"] * len(spans)
    for k, st in enumerate(case["builds"]):
        ev = case["events"][k - 1] if k else dict(kind="none", clean=0)
        for i, (m, (r0, r1)) in enumerate(zip(maps, spans)):
            if k and ev["clean"] == 0 and ev["kind"] in ("mutator", "centre", "bind_out", "unbind_out"):
                m.invalidate()
                why[i] = {"bind_out": "output", "unbind_out": "output"}.get(ev["kind"], ev["kind"])
            old = m.flags.copy()
            was_known = m.known
            mode, stored, neg = m.build(st, [im[r0:r1] for im in imgs[k]])
            rec = dict(k=k, band=i, span=(r0, r1), mode=mode, stored=stored, neg=neg, old=old,
                       after=why[i] if mode == 1 else None, poisoned=ev["kind"] == "poison", known_before=was_known,
                       known_after=m.known)
            if mode == 0:
                why[i] = ("uint8 build" if st["k_keep"] else "keep_kernel 0 build" if st["kept"] and st["eligible"]
                          else "ineligible build" if st["kept"] else why[i])  # a full build: the event's reason stays
            yield rec
            if ev["kind"] == "poison" and poison_rebuild:
                m.invalidate()  # gdp_pyramid_written, then a full build
                why[i] = "poison"
