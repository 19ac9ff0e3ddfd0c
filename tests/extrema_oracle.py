"""Shared by the extrema tests (a plain module, no fixtures): the numpy float32 oracle that implements
the keypoint rules of include/gdp.h literally, the helpers that compare record sets exactly, the
pyramid generators, and the "one neighbour decides" lattice pyramids whose keypoints are known in
closed form, without the oracle.  tests/test_extrema_oracle.py checks the oracle itself on the CPU."""
import ctypes
import functools

import numpy as np

F = np.float32


# ---------------------------------------------------------------------------------------------
# the oracle
# ---------------------------------------------------------------------------------------------
def octave_levels(packed, H, W, S, O):
    """Views [S+3][rows][cols] of every octave of a packed [o][s][rows][cols] pyramid."""
    out, off = [], 0
    for o in range(O):
        r, c = H >> o, W >> o
        out.append(packed[off:off + (S + 3) * r * c].reshape(S + 3, r, c))
        off += (S + 3) * r * c
    assert off == packed.size
    return out


def np_extrema(packed, H, W, S, O, contrast=0.0, edge_ratio=0.0):
    """(set of (octave, scale, kind, row, col, value bits), contrast-passing extrema before the
    edge test)."""
    found, before_edge = set(), 0
    er = F(edge_ratio)
    with np.errstate(all="ignore"):
        for o, D in enumerate(octave_levels(packed, H, W, S, O)):
            rows, cols = D.shape[1:]
            if S == 0 or rows < 3 or cols < 3:
                continue
            for s in range(1, S + 1):  # level S+2 is never read
                v = D[s, 1:-1, 1:-1]
                gt = np.ones(v.shape, bool)
                lt = np.ones(v.shape, bool)
                for ds in (-1, 0, 1):
                    for dr in (-1, 0, 1):
                        for dc in (-1, 0, 1):
                            if (ds, dr, dc) != (0, 0, 0):
                                n = D[s + ds, 1 + dr:rows - 1 + dr, 1 + dc:cols - 1 + dc]
                                gt &= v > n
                                lt &= v < n
                keep = (gt | lt) & (np.abs(v) > F(contrast))
                before_edge += int(keep.sum())
                if edge_ratio != 0:
                    d = lambda dr, dc: D[s, 1 + dr:rows - 1 + dr, 1 + dc:cols - 1 + dc]  # noqa: E731
                    dxx = (d(0, 1) + d(0, -1)) - F(2) * v
                    dyy = (d(1, 0) + d(-1, 0)) - F(2) * v
                    dxy = ((d(1, 1) - d(1, -1)) - (d(-1, 1) - d(-1, -1))) * F(0.25)
                    tr = dxx + dyy
                    det = dxx * dyy - dxy * dxy
                    assert det.dtype == np.float32 and tr.dtype == np.float32
                    keep &= (det > F(0)) & ((tr * tr) * er < ((er + F(1)) * (er + F(1))) * det)
                for r, c in zip(*np.nonzero(keep)):
                    val = v[r, c]
                    found.add((o, s, 1 if gt[r, c] else -1, int(r) + 1, int(c) + 1, int(val.view(np.uint32))))
    return found, before_edge


def as_set(kp):
    kp = np.asarray(kp)
    got = set(zip(*(kp[f].tolist() for f in ("octave", "scale", "kind", "row", "col")), kp["value"].view(np.uint32).tolist()))
    assert len(got) == len(kp), "duplicate records"
    return got


def assert_sorted(kp):
    keys = [(int(k["octave"]), int(k["scale"]), int(k["row"]), int(k["col"])) for k in kp]
    assert keys == sorted(keys)


def assert_short_downloads(download, full, found=True):
    """`download(host, capacity, stored, found)` calls a stage's gdp_download_* export on a list whose whole
    sorted download is `full`.  Through a buffer shorter than the list: stored == capacity, found == the
    full count, and the records are the first `capacity` of `full`.  With host NULL and capacity 0:
    GDP_OK, nothing stored, found still the full count."""
    assert len(full) >= 2
    for capacity in (len(full) - 1, 0):  # one record short: the one left out is the sorted list's last
        part = np.zeros(len(full), full.dtype)
        stored, total = ctypes.c_size_t(99), ctypes.c_size_t(99)
        host = ctypes.c_void_p(part.ctypes.data) if capacity else None
        assert download(host, capacity, ctypes.byref(stored), ctypes.byref(total)) == 0
        assert stored.value == capacity and part[:capacity].tobytes() == np.asarray(full)[:capacity].tobytes()
        assert not part[capacity:].tobytes().strip(b"\0")  # nothing beyond the buffer's capacity
        assert not found or total.value == len(full)


SMALL_IMAGE = (64, 96, 2, 4242)  # H, W, S, seed of the LCG image the list-handling edge cases run on


def small_pipeline(pkg, oracle, stages):
    """A context on the small image, built, with the first `stages` of detect, refine, orient, describe run."""
    H, W, S, seed = SMALL_IMAGE
    ctx = pkg.PyramidContext(H, W, S=S)
    ctx.set_input(oracle.lcg_image(H, W, seed))
    ctx.build()
    for run in (ctx.detect_extrema, ctx.refine_keypoints, ctx.orient_keypoints, ctx.describe_keypoints)[:stages]:
        run()
    return ctx


def packed_size(H, W, S, O):
    return sum((S + 3) * (H >> o) * (W >> o) for o in range(O))


def detect(pkg, packed, H, W, S, octaves=0, contrast=0.0, edge_ratio=0.0, capacity=None):
    with pkg.PyramidContext(H, W, S=S, octaves=octaves) as ctx:
        if capacity:
            ctx.set_keypoint_capacity(capacity)
        ctx.upload_pyramid(packed)
        ctx.detect_extrema(contrast, edge_ratio)
        kp = ctx.keypoints(0)
        assert kp.found == ctx.keypoint_count(0)
        assert_sorted(kp)
        return kp


# ---------------------------------------------------------------------------------------------
# shared inputs (computed once, never modified)
# ---------------------------------------------------------------------------------------------
BIG = (200, 520, 2, 8)     # all 8 octaves; ~20 k keypoints: every seam of any tiling is hit
ODD = (37, 100, 3, 6)      # odd widths (octave-2 cols = 25), unaligned rows, 4x12 / 2x6 / 1x3 octaves


@functools.lru_cache(maxsize=None)
def normal_pyramid(shape):
    H, W, S, O = shape
    p = np.random.default_rng(7).standard_normal(packed_size(H, W, S, O), dtype=np.float32)
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def tie_pyramid(shape):
    """Integers in [-3, 3] (ties everywhere) with a few hundred NaN, +-inf, +-0 and denormals."""
    H, W, S, O = shape
    rng = np.random.default_rng(7)
    p = rng.integers(-3, 4, packed_size(H, W, S, O)).astype(np.float32)
    special = np.array([np.nan, -np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-45, -1e-45, 1e-39, -1e-39], np.float32)
    where = rng.choice(p.size, 400, replace=False)
    p[where] = special[rng.integers(0, special.size, where.size)]
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def smooth_pyramid(shape):
    """normal_pyramid box-filtered along rows with 5 taps (edge rows repeated)."""
    H, W, S, O = shape
    out = np.empty_like(normal_pyramid(shape))
    for src, dst in zip(octave_levels(normal_pyramid(shape), H, W, S, O), octave_levels(out, H, W, S, O)):
        pad = np.pad(src, ((0, 0), (0, 0), (2, 2)), mode="edge")
        acc = np.zeros_like(src)
        for k in range(5):
            acc = acc + pad[:, :, k:k + src.shape[2]]
        dst[...] = acc * F(0.2)
    out.setflags(write=False)
    return out


DENORMAL_ULP = F(2.0 ** -149)  # the smallest float32 denormal


@functools.lru_cache(maxsize=None)
def one_signed_pyramid(shape, sign):
    """Uniform values in [1, 2) times `sign`: a stray 0 (or any value of the other sign) used as a
    neighbour blocks every maximum (sign +1) or minimum (-1) next to it."""
    H, W, S, O = shape
    p = (F(1) + np.random.default_rng(13).random(packed_size(H, W, S, O), dtype=np.float32)) * F(sign)
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def denormal_pyramid(shape, spread):
    """Random integers in [-spread, spread] times 2^-149: every value is a denormal (or +0).
    spread = 2^20 gives practically distinct values, spread = 3 ties everywhere.  On a host whose
    FPU flushes denormals the product is all zeros, which the assertion below refuses."""
    H, W, S, O = shape
    assert spread < 2 ** 23
    k = np.random.default_rng(17).integers(-spread, spread + 1, packed_size(H, W, S, O))
    p = k.astype(np.float32) * DENORMAL_ULP
    assert np.array_equal(p.view(np.uint32) & np.uint32(0x7FFFFFFF), np.abs(k).astype(np.uint32)), \
        "the host does not keep float32 denormals"
    p.setflags(write=False)
    return p


_KINDS = {"normal": normal_pyramid, "tie": tie_pyramid, "smooth": smooth_pyramid}


@functools.lru_cache(maxsize=None)
def want(kind, shape, contrast=0.0, edge_ratio=0.0):
    return np_extrema(_KINDS[kind](shape), *shape, contrast=contrast, edge_ratio=edge_ratio)


# ---------------------------------------------------------------------------------------------
# "one neighbour decides" lattice pyramids
# ---------------------------------------------------------------------------------------------
HI = F(1.0)
LO = np.nextafter(F(1.0), F(0.0))  # one ulp below HI
# the 26 neighbour directions (ds, dr, dc) in lexicographic order; index 26 is "no neighbour"
DIRECTIONS = tuple((ds, dr, dc) for ds in (-1, 0, 1) for dr in (-1, 0, 1) for dc in (-1, 0, 1)
                   if (ds, dr, dc) != (0, 0, 0))
_OFFSETS = np.array(DIRECTIONS + ((0, 0, 0),))
PHASES = tuple((ps, pr, pc) for ps in range(3) for pr in range(3) for pc in range(3))


def lattice_octave(D, S, phase, rho, sigma, o=0):
    """Fill D, the [S+3][rows][cols] levels of octave o, with the lattice of the given phase in
    {0,1,2}^3, rotation rho in 0..26 and sign sigma in {+1, -1}; returns its keypoints.

    Everything is LO = 1 - ulp except level S+2, which is NaN (it is never read).  Centres sit every
    3 samples in scale, row and column, starting at (1, 1, 1) + phase, and hold HI = 1: each is a
    strict maximum by exactly one ulp.  With i, j the ordinals of a centre's row and column and
    d = (i + j + s + o + rho) mod 27, the neighbour in DIRECTIONS[d] is raised to HI as well when
    d < 26: that one tie decides that the centre is no keypoint.  For d == 26 nothing blocks it.
    Centres are 3 apart on every axis, so no raised neighbour is within reach of another centre,
    and every other candidate ties with a LO neighbour.  Finally all values are multiplied by
    sigma (-1 turns the maxima into minima)."""
    ps, pr, pc = phase
    rows, cols = D.shape[1:]
    assert D.shape[0] == S + 3 and 0 <= rho < 27 and sigma in (1, -1)
    D[...] = LO
    D[S + 2] = np.nan
    s, r, c = np.meshgrid(np.arange(1 + ps, S + 1, 3), np.arange(1 + pr, rows - 1, 3), np.arange(1 + pc, cols - 1, 3),
                          indexing="ij")
    d = ((r - 1 - pr) // 3 + (c - 1 - pc) // 3 + s + o + rho) % 27
    off = _OFFSETS[d]
    D[s, r, c] = HI
    D[s + off[..., 0], r + off[..., 1], c + off[..., 2]] = HI  # d == 26 rewrites the centre itself
    D *= F(sigma)
    bits = int(F(sigma * HI).view(np.uint32))
    free = d == 26
    return {(o, int(a), sigma, int(b), int(e), bits) for a, b, e in zip(s[free], r[free], c[free])}


def lattice_pyramid(H, W, S, O, phase, rho, sigma):
    """(packed pyramid, its keypoints in closed form): lattice_octave on every octave."""
    packed = np.empty(packed_size(H, W, S, O), np.float32)
    expect = set()
    for o, D in enumerate(octave_levels(packed, H, W, S, O)):
        expect |= lattice_octave(D, S, phase, rho, sigma, o)
    return packed, expect
