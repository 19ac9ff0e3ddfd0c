"""CPU-only: the shapes of tests/test_gpu_keep_support.py really have what they are chosen for,
worked out from steady_cases._support and the 16 x 256 tile grid (tests/keep_support_cases.py)."""
from keep_support_cases import SHAPES, group_rects, slow_tiles, span, support_units, tail_units, tiles
from steady_cases import FUSED, TILE_COLS, TILE_ROWS, _support


def _grid(name):
    W = SHAPES[name][1]
    r0, r1 = span(name)
    return -(-(r1 - r0) // TILE_ROWS), -(-W // TILE_COLS)


def test_slow_tiles_are_rectangles_and_every_shape_has_support_units(oracle):
    for name in SHAPES:
        for trs, tcs in slow_tiles(oracle, name):
            assert trs == list(range(trs[0], trs[-1] + 1)) if trs else not tcs
            assert tcs == list(range(tcs[0], tcs[-1] + 1)) if tcs else not trs
        assert support_units(oracle, name) > 0, name
        assert len(slow_tiles(oracle, name)) == FUSED  # every shape fuses five octaves


def test_some_octave_has_fast_and_slow_tiles_in_each_direction(oracle):
    """200x1028 and the band: tile rows and tile columns on both sides of the test, in several octaves."""
    for name in ("200x1028", "band_128_256"):
        tiles_r, tiles_c = _grid(name)
        both = [o for o, (trs, tcs) in enumerate(slow_tiles(oracle, name))
                if 0 < len(trs) < tiles_r and 0 < len(tcs) < tiles_c]
        assert both, name
        if name == "200x1028":
            assert len(both) >= 2, both
    # and a rectangle that starts at neither edge, in rows and in columns
    trs, tcs = slow_tiles(oracle, "200x1028")[0]
    tiles_r, tiles_c = _grid("200x1028")
    assert trs[0] > 0 and trs[-1] < tiles_r - 1 and tcs[0] > 0 and tcs[-1] < tiles_c - 1


def test_some_octave_has_a_slow_rectangle_of_at_least_2_by_2_tiles(oracle):
    for name in ("200x1028", "96x768_b3", "64x2048_o7", "band_128_256"):
        assert any(len(trs) >= 2 and len(tcs) >= 2 for trs, tcs in slow_tiles(oracle, name)), name


def test_some_octave_has_a_tile_footprint_of_a_single_row(oracle):
    """Octave 4 of a 16-row tile is one row: slow tiles there in every shape, and in 48x520 rectangles
    of several tile rows whose rows are one per tile."""
    assert TILE_ROWS >> (FUSED - 1) == 1
    for name in SHAPES:
        trs, tcs = slow_tiles(oracle, name)[FUSED - 1]
        assert trs and tcs, name
        _, rows, _, gpr = group_rects(oracle, name)[FUSED - 1]
        assert rows == len(trs) and gpr > 0, name


def test_48x520_seam_narrow_last_column_and_rows_inside_the_support(oracle):
    H, W, O, S, _ = SHAPES["48x520"]
    tiles_r, tiles_c = _grid("48x520")
    assert W - (tiles_c - 1) * TILE_COLS == 8  # the last tile column is 8 pixels wide
    rows0, cols0 = _support(oracle, H, W, O, S)[0]
    assert rows0.all()  # every row of octave 0 is inside the support
    nz = cols0.nonzero()[0]
    assert nz[0] < TILE_COLS <= nz[-1]  # the column support crosses the seam between tile columns 0 and 1
    # both tile columns at the seam are slow in every octave; the narrow column is fast in every octave (its footprint
    # in octave 4, clipped to the octave's 32 columns, is empty), so the group rectangles stop short of the width
    for o, (trs, tcs) in enumerate(slow_tiles(oracle, "48x520")):
        assert len(trs) == tiles_r and tcs == [0, 1], o
    assert tiles_c == 3


def test_small_batched_tail_and_band_shapes(oracle):
    assert _grid("64x96") == (4, 1) and SHAPES["64x96"][1] < TILE_COLS  # smaller than a tile in width
    for o, (_, rows, c0, gpr) in enumerate(group_rects(oracle, "64x96")):  # the rectangles are clipped to the width
        assert c0 == 0 and gpr == -(-(96 >> o) // 4) and 4 * gpr < TILE_COLS >> o, o
    # batch 3: the groups of one image are no multiple of a unit, so units straddle images
    per = sum(rows * gpr for _, rows, _, gpr in group_rects(oracle, "96x768_b3"))
    assert per % 256 != 0 and support_units(oracle, "96x768_b3") < 3 * -(-per // 256) + 1
    assert SHAPES["96x768_b3"][4]["batch"] == 3
    # support units and tail units in one launch
    assert support_units(oracle, "64x2048_o7") > 0 and tail_units("64x2048_o7") > 0 and tiles("64x2048_o7") > 0
    # the band: its first row is not the image's, and some octave's support starts above or ends below it
    r0, r1 = span("band_128_256")
    assert r0 > 0 and r1 < SHAPES["band_128_256"][0]
    rects = group_rects(oracle, "band_128_256")
    assert all(rows > 0 for _, rows, _, _ in rects)
    # an octave whose slow tile rows do not start at the band's first tile row, or stop before its last
    tiles_r, _ = _grid("band_128_256")
    assert any(trs and (trs[0] > 0 or trs[-1] < tiles_r - 1) for trs, _ in slow_tiles(oracle, "band_128_256"))
