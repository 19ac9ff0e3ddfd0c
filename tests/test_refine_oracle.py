"""The refinement oracle (tests/refine_oracle.py) checked on the CPU, without the library: closed-form
quadratic pyramids on which every step of the rule of gdp_refine_keypoints is exact, and the
coverage the GPU tests rely on — the shared pyramids reach every outcome of the rule."""
from collections import Counter

import numpy as np

from extrema_oracle import BIG, ODD, F, smooth_pyramid, tie_pyramid
from refine_oracle import (MAX_STEPS, REASONS, extrema_records, np_refine, quad_expect, quad_pyramid, records)

S, ROWS, COLS = 5, 24, 40
CENTRE = (3.25, 10.125, 20.5)
# start -> (final sample, moves); the first six converge, the last two need a sixth solve
STARTS = {(3, 10, 20): ((3, 10, 20), 0), (5, 10, 20): ((3, 10, 20), 2), (1, 14, 17): ((3, 10, 20), 4),
          (3, 10, 21): ((3, 10, 21), 0), (3, 12, 24): ((3, 10, 21), 3), (3, 10, 25): ((3, 10, 21), 4),
          (3, 10, 26): None, (3, 16, 20): None}


def bits(x):
    return int(F(x).view(np.uint32))


def refine_quad(D, starts, **kw):
    moves = []
    kept, why = np_refine(D.ravel(), D.shape[1], D.shape[2], D.shape[0] - 3, 1, records(starts), moves_out=moves, **kw)
    return kept, why, moves


def test_quadratic_is_exact_in_float32():
    D = quad_pyramid(S, ROWS, COLS, *CENTRE)
    assert D.dtype == np.float32 and D.shape == (S + 3, ROWS, COLS)
    assert D[3, 10, 20] == F(64 - 0.5 * 0.25 - 0.25 * 0.015625 - 0.0625)
    assert MAX_STEPS == 5 and REASONS == ("ok", "singular", "nan", "left", "steps", "contrast", "edge")


def test_eight_starts_closed_form():
    D = quad_pyramid(S, ROWS, COLS, *CENTRE)
    starts = list(STARTS)
    kept, why, moves = refine_quad(D, starts)
    assert why == ["ok"] * 6 + ["steps"] * 2
    assert moves[:6] == [0, 2, 4, 0, 3, 4]
    expect = []
    for st in starts[:6]:
        (s, r, c), _ = STARTS[st]
        dcol = 0.5 if c == 20 else -0.5
        expect.append((0, s, 1, r, c, int(D[s, r, c].view(np.uint32)), bits(0.25), bits(0.125), bits(dcol), bits(64.0)))
        assert quad_expect(st, *CENTRE, S, ROWS, COLS) == ((s, r, c), (0.25, 0.125, dcol), STARTS[st][1])
    assert kept == sorted(expect)  # a multiset: three identical records at each of the two samples
    assert Counter(kept).most_common(1)[0][1] == 3
    assert all(quad_expect(st, *CENTRE, S, ROWS, COLS) is None for st in starts[6:])


def test_each_start_alone_gives_its_record():
    D = quad_pyramid(S, ROWS, COLS, *CENTRE)
    for st, want in STARTS.items():
        kept, why, _ = refine_quad(D, [st])
        assert (len(kept) == 1 and kept[0][1:2] + kept[0][3:5] == want[0]) if want else (kept == [] and why == ["steps"]), st


def test_contrast_and_edge_on_the_quadratic():
    D = quad_pyramid(S, ROWS, COLS, *CENTRE)
    st = [(3, 10, 20)]
    assert refine_quad(D, st, contrast=63.9375)[1] == ["ok"]  # interp is exactly 64
    assert refine_quad(D, st, contrast=64.0)[1] == ["contrast"]  # strictly above
    # dxx = -2a = -1, dyy = -2b = -0.5: tr^2 / det = 2.25 / 0.5 = 4.5 = (r+1)^2 / r at r = 2
    assert refine_quad(D, st, edge_ratio=2.0)[1] == ["edge"]  # strictly below
    assert refine_quad(D, st, edge_ratio=2.125)[1] == ["ok"]
    saddle = quad_pyramid(S, ROWS, COLS, *CENTRE, b=-0.25)  # det of the 2 x 2 Hessian < 0
    assert refine_quad(saddle, st)[1] == ["ok"] and refine_quad(saddle, st, edge_ratio=10.0)[1] == ["edge"]


def test_mixed_term_still_converges_at_the_centre():
    D = quad_pyramid(S, ROWS, COLS, *CENTRE, mix=0.125)
    kept, why, moves = refine_quad(D, [(3, 10, 20), (3, 12, 23)])
    assert why == ["ok", "ok"] and moves[0] == 0 and moves[1] >= 2
    for t in kept:
        off = [float(np.uint32(x).view(np.float32)) for x in t[6:9]]
        pos = [t[1] + off[0], t[3] + off[1], t[4] + off[2]]
        assert np.allclose(pos, CENTRE, atol=1e-5) and abs(float(np.uint32(t[9]).view(np.float32)) - 64.0) < 1e-4


def test_walks_out_of_each_face():
    for centre in [(3.25, 10.125, -3.0), (3.25, 10.125, COLS + 2.0), (3.25, -3.0, 20.5), (3.25, ROWS + 2.0, 20.5),
                   (-1.0, 10.125, 20.5), (S + 3.0, 10.125, 20.5)]:
        D = quad_pyramid(S, ROWS, COLS, *centre)
        near = [(2 if centre[0] < 1 else S - 1 if centre[0] > S else 3),
                (2 if centre[1] < 1 else ROWS - 3 if centre[1] > ROWS - 2 else 10),
                (2 if centre[2] < 1 else COLS - 3 if centre[2] > COLS - 2 else 20)]
        kept, why, moves = refine_quad(D, [tuple(near)])
        assert kept == [] and why == ["left"] and moves == [2], centre
        assert quad_expect(tuple(near), *centre, S, ROWS, COLS) is None


def test_level_s_plus_2_is_never_read():
    D = quad_pyramid(S, ROWS, COLS, S + 0.25, 10.125, 20.5)
    D[S + 2] = np.nan
    kept, why, _ = refine_quad(D, [(S, 10, 20), (S - 2, 10, 20)])
    assert why == ["ok", "ok"] and [t[1] for t in kept] == [S, S]
    assert all(t[6:10] == (bits(0.25), bits(0.125), bits(0.5), bits(64.0)) for t in kept)


def test_singular_and_nan_offsets():
    flat = np.full((S + 3, 8, 8), 1.0, np.float32)
    assert refine_quad(flat, [(2, 3, 3)])[1] == ["singular"]  # det = 0
    flat[2, 3, 3] = np.nan
    assert refine_quad(flat, [(2, 3, 3)])[1] == ["singular"]  # det = NaN
    # a finite determinant with an infinite gradient: every offset is NaN, nothing moves
    D = quad_pyramid(S, 8, 8, 2.0, 3.0, 3.0)
    D[2, 3, 4] = np.float32(3e38)
    D[2, 3, 2] = np.float32(-3e38)
    kept, why, _ = refine_quad(D, [(2, 3, 3)])
    assert kept == [] and why[0] in ("nan", "singular")


# ---------------------------------------------------------------------------------------------
# coverage of the shared pyramids (what tests/test_gpu_refine.py relies on)
# ---------------------------------------------------------------------------------------------
def test_smooth_pyramid_reaches_every_outcome():
    rec = extrema_records("smooth", BIG)
    moves = []
    kept, why = np_refine(smooth_pyramid(BIG), *BIG, rec, 0.3, 10.0, moves_out=moves)
    n = Counter(why)
    stay = sum(1 for w, m in zip(why, moves) if w == "ok" and m == 0)
    moved = sum(1 for w, m in zip(why, moves) if w == "ok" and m >= 1)
    print(len(rec), stay, moved, dict(n))
    assert len(rec) > 10000 and len(kept) == n["ok"] == stay + moved
    assert min(stay, moved, n["left"], n["steps"], n["contrast"], n["edge"]) > 0
    assert max(moves) <= MAX_STEPS


def test_tie_pyramids_reach_singular_and_nan():
    for shape in (BIG, ODD):
        kept, why = np_refine(tie_pyramid(shape), *shape, extrema_records("tie", shape))
        n = Counter(why)
        print(shape, dict(n))
        assert n["singular"] > 0 and n["nan"] > 0 and n["ok"] == len(kept) > 0


def test_no_nan_in_kept_records():
    """A kept record passed |x| <= 0.5 and |interp| > contrast, so its offsets and interp are numbers;
    its bit patterns are then unique per value and the multiset comparison is meaningful."""
    for shape in (BIG, ODD):
        kept, _ = np_refine(tie_pyramid(shape), *shape, extrema_records("tie", shape))
        vals = np.array([t[6:10] for t in kept], np.uint32).view(np.float32)
        assert not np.isnan(vals).any() and (np.abs(vals[:, :3]) <= 0.5).all()
