"""The judge of the extrema kernel is itself judged (CPU only): np_extrema, vectorised numpy with its
own slicing arithmetic, against (a) a literal scalar implementation of the rules of include/gdp.h —
one candidate, one neighbour, one float32 comparison at a time — and (b) the lattice pyramids of
tests/extrema_oracle.py, whose keypoints are known in closed form."""
import numpy as np
import pytest

from extrema_oracle import (DENORMAL_ULP, DIRECTIONS, PHASES, F, lattice_pyramid, np_extrema, octave_levels,
                            packed_size)


def scalar_extrema(packed, H, W, S, O, contrast=0.0, edge_ratio=0.0):
    """gdp.h's rules 1-3 read out literally.  Returns (keypoints, statistics): `nan_disqualified`
    counts candidates that a NaN among their 27 values disqualifies although they are strictly
    above or below every other neighbour, `ties` candidates that are >= (or <=) all 26 neighbours
    but equal to one of them."""
    found, stats = set(), {"nan_disqualified": 0, "ties": 0}
    thr, er = F(contrast), F(edge_ratio)
    with np.errstate(all="ignore"):
        for o, D in enumerate(octave_levels(packed, H, W, S, O)):
            rows, cols = D.shape[1:]
            for s in range(1, S + 1):
                for r in range(1, rows - 1):
                    for c in range(1, cols - 1):
                        v = D[s, r, c]
                        gt = lt = ge = le = gt_seen = lt_seen = True
                        nans = int(np.isnan(v))
                        for ds, dr, dc in DIRECTIONS:
                            n = D[s + ds, r + dr, c + dc]
                            gt = gt and bool(v > n)
                            lt = lt and bool(v < n)
                            ge = ge and bool(v >= n)
                            le = le and bool(v <= n)
                            if np.isnan(n):
                                nans += 1
                            else:  # what the verdict would be without the NaN neighbours
                                gt_seen = gt_seen and bool(v > n)
                                lt_seen = lt_seen and bool(v < n)
                        if nans and not np.isnan(v) and (gt_seen or lt_seen):
                            stats["nan_disqualified"] += 1
                        if (ge and not gt) or (le and not lt):
                            stats["ties"] += 1
                        if not (gt or lt):
                            continue
                        if not (np.abs(v) > thr):
                            continue
                        if edge_ratio != 0:
                            d = D[s]
                            dxx = (d[r, c + 1] + d[r, c - 1]) - F(2) * v
                            dyy = (d[r + 1, c] + d[r - 1, c]) - F(2) * v
                            dxy = ((d[r + 1, c + 1] - d[r + 1, c - 1]) - (d[r - 1, c + 1] - d[r - 1, c - 1])) * F(0.25)
                            tr = dxx + dyy
                            det = dxx * dyy - dxy * dxy
                            assert type(tr) is np.float32 and type(det) is np.float32
                            if not (det > F(0) and (tr * tr) * er < ((er + F(1)) * (er + F(1))) * det):
                                continue
                        found.add((o, s, 1 if gt else -1, r, c, int(v.view(np.uint32))))
    return found, stats


SPECIAL = np.array([np.nan, -np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-45, -1e-45, 1e-39, -1e-39], np.float32)


def small_pyramid(kind, H, W, S, O):
    rng = np.random.default_rng(S)
    size = packed_size(H, W, S, O)
    if kind == "ties":  # integers in [-3, 3], mostly small: ties everywhere, and rare +-2 that are keypoints
        p = rng.choice(np.arange(-3, 4), size, p=[0.01, 0.03, 0.26, 0.40, 0.26, 0.03, 0.01]).astype(np.float32)
        nspecial = size // 25
    elif kind == "normal":  # many strict extrema, a quarter of them next to a NaN
        p = (F(1.5) * rng.standard_normal(size, dtype=np.float32)).astype(np.float32)
        nspecial = size // 50
    else:  # distinct denormals: the centre of every keypoint is one
        p = (rng.permutation(size) - size // 2).astype(np.float32) * DENORMAL_ULP
        nspecial = 0
    where = rng.choice(size, nspecial, replace=False)
    p[where] = SPECIAL[rng.integers(0, SPECIAL.size, nspecial)]
    return p


@pytest.mark.parametrize("S", [1, 2, 4])
@pytest.mark.parametrize("kind", ["ties", "normal", "denormal"])
def test_oracle_equals_the_scalar_rules(kind, S):
    H, W, O = 19, 30, 3  # octaves 19 x 30, 9 x 15, 4 x 7: odd and even sizes
    p = small_pyramid(kind, H, W, S, O)
    for contrast in (0.0, 2.0):
        for edge_ratio in (0.0, 1.5):
            want, stats = scalar_extrema(p, H, W, S, O, contrast, edge_ratio)
            got, _ = np_extrema(p, H, W, S, O, contrast, edge_ratio)
            assert got == want, (contrast, edge_ratio)
            if (contrast, edge_ratio) != (0.0, 0.0):
                continue
            # the comparison is not vacuous
            assert want and {k[1] for k in want} == set(range(1, S + 1)) and {k[2] for k in want} == {1, -1}
            if kind != "ties":  # (strict extrema of the tie pyramid are too rare for the 7 x 13 candidates of octave 1)
                assert {k[0] for k in want} >= {0, 1}
            if kind == "ties":
                assert stats["ties"] > 20 and np.isnan(p).any() and np.isinf(p).any()
                assert any((k[5] & 0x7FFFFFFF) == int(F(2).view(np.uint32)) for k in want)  # contrast 2 meets |v| == 2
            if kind == "normal":
                assert stats["nan_disqualified"] >= 1
            if kind == "denormal":
                assert all(0 < (k[5] & 0x7FFFFFFF) < 0x00800000 for k in want)
                assert not np_extrema(p, H, W, S, O, 2.0)[0]


# every path of the kernel's geometry in miniature, plus one shape with two 248-column strips
LATTICE_SHAPES = [(3, 3, 1, 1), (4, 5, 2, 1), (7, 9, 3, 1), (8, 6, 4, 1), (20, 9, 7, 1), (19, 250, 3, 1), (12, 13, 2, 2)]


@pytest.mark.parametrize("shape", LATTICE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_oracle_equals_the_lattice_closed_form(shape):
    H, W, S, O = shape
    big = H * W > 1000
    total = set()
    for phase in PHASES:
        for rho in ((0, 5, 26) if big else range(27)):
            for sigma in (1, -1):
                p, expect = lattice_pyramid(H, W, S, O, phase, rho, sigma)
                assert np_extrema(p, H, W, S, O)[0] == expect, (phase, rho, sigma)
                total |= expect
    if not big:  # over all rotations and phases every candidate is a keypoint once per sign
        cand = sum(S * ((H >> o) - 2) * ((W >> o) - 2) for o in range(O) if (H >> o) >= 3 and (W >> o) >= 3)
        assert len(total) == 2 * cand


def test_lattice_raises_every_direction_once_per_centre():
    """Over rho = 0..26 one fixed centre sees each of its 26 neighbours raised exactly once and is
    left unblocked exactly once."""
    H, W, S = 7, 8, 3
    hi = int(F(1).view(np.uint32))
    seen = []
    for rho in range(27):
        p, expect = lattice_pyramid(H, W, S, 1, (1, 2, 0), rho, 1)
        D = octave_levels(p, H, W, S, 1)[0]
        s, r, c = 2, 3, 4  # the centre with ordinals (0, 0, 1) of phase (1, 2, 0)
        assert int(D[s, r, c].view(np.uint32)) == hi
        raised = [d for d in DIRECTIONS if int(D[s + d[0], r + d[1], c + d[2]].view(np.uint32)) == hi]
        assert len(raised) <= 1 and ((0, s, 1, r, c, hi) in expect) == (not raised)
        seen.append(raised[0] if raised else None)
    assert sorted(seen, key=str) == sorted(list(DIRECTIONS) + [None], key=str)


def test_as_set_and_assert_sorted_read_every_field():
    """The record helpers keep sign, NaN payload and -0 of the value bits and refuse duplicates."""
    from extrema_oracle import as_set, assert_sorted

    dt = np.dtype({"names": ["octave", "scale", "kind", "row", "col", "value"],
                   "formats": [np.uint16, np.uint8, np.int8, np.int32, np.int32, np.float32],
                   "offsets": [0, 2, 3, 4, 8, 12], "itemsize": 16})
    kp = np.zeros(4, dt)
    kp[0] = (0, 1, 1, 2, 3, 1.5)
    kp[1] = (0, 1, -1, 2, 4, -0.0)
    kp[2] = (0, 2, -1, 1, 1, -np.inf)
    kp[3] = (300, 7, 1, 70000, 1, 1e-45)
    want = {(0, 1, 1, 2, 3, 0x3FC00000), (0, 1, -1, 2, 4, 0x80000000), (0, 2, -1, 1, 1, 0xFF800000), (300, 7, 1, 70000, 1, 1)}
    assert as_set(kp) == want
    assert as_set(kp[:0]) == set()
    assert_sorted(kp)
    with pytest.raises(AssertionError):
        assert_sorted(kp[::-1])
    with pytest.raises(AssertionError, match="duplicate"):
        as_set(kp[[0, 1, 0]])
