"""Shared by the support-unit tests (a plain module, no fixtures, no GPU): the shapes of
tests/test_gpu_keep_support.py and a model of k_keep's support units (GDP_TUNE_KEEP_SUPPORT,
csrc/gdp_keep.inc) worked out from steady_cases._support and the 16 x 256 tile grid alone.

Per fused octave the tiles whose footprint meets the support's bounding ranges — the hit test of
steady_cases.clean_tiles — form a rectangle of tiles; the octave's footprint of that rectangle,
clipped to the rows and columns the context holds, is a rectangle of 4-pixel groups; a support unit
is 256 consecutive groups of those rectangles, flattened per image over the batch.
tests/test_keep_support_cases.py checks on the CPU that the shapes have what they are chosen for.
"""
from steady_cases import FUSED, TAIL_GROUPS, TILE_COLS, TILE_ROWS, _support

# name: H, W, octaves, S, context keywords
SHAPES = {
    "48x520": (48, 520, 5, 2, {}),          # support across a tile-column seam, a last tile column 8 pixels wide,
                                            # rows all inside the support
    "200x1028": (200, 1028, 5, 2, {}),      # fast and slow tile rows and columns in several octaves
    "64x96": (64, 96, 5, 2, {}),            # smaller than a tile
    "96x768_b3": (96, 768, 5, 2, dict(batch=3)),   # the per-image flattening
    "64x2048_o7": (64, 2048, 7, 2, {}),     # support units and tail units in one launch
    "band_128_256": (384, 1028, 5, 2, dict(row_begin=128, row_end=256)),  # a row band, row0 != 0
}


def span(name):
    H, kw = SHAPES[name][0], SHAPES[name][4]
    return kw.get("row_begin", 0), kw.get("row_end", H)


def _box(mask):
    nz = mask.nonzero()[0]
    return (int(nz[0]), int(nz[-1]) + 1) if nz.size else (0, 0)


def slow_tiles(oracle, name):
    """Per fused octave: (tile rows, tile columns) — sorted lists of the band-local tile rows whose
    footprint meets the support's row range and of the tile columns that meet its column range.  A
    (tile, octave) pair is slow iff its row is in the first and its column in the second."""
    H, W, O, S, _ = SHAPES[name]
    r0, r1 = span(name)
    out = []
    for o, (rows, cols) in enumerate(_support(oracle, H, W, O, S)[:FUSED]):
        (sr0, sr1), (sc0, sc1) = _box(rows), _box(cols)
        trs, tcs = [], []
        for tr in range(-(-(r1 - r0) // TILE_ROWS)):
            r_lo = (r0 >> o) + (tr * TILE_ROWS >> o)
            if r_lo < sr1 and r_lo + (TILE_ROWS >> o) > sr0:
                trs.append(tr)
        for tc in range(-(-W // TILE_COLS)):
            c_lo = tc * TILE_COLS >> o
            if c_lo < sc1 and min(c_lo + (TILE_COLS >> o), W >> o) > sc0:
                tcs.append(tc)
        out.append((trs, tcs) if trs and tcs else ([], []))
    return out


def group_rects(oracle, name):
    """Per fused octave: (first band-local row, rows, first column, groups per row) of the slow
    tiles' footprint in that octave, clipped to the rows the context holds and the octave's width."""
    H, W, _, _, _ = SHAPES[name]
    r0, r1 = span(name)
    out = []
    for o, (trs, tcs) in enumerate(slow_tiles(oracle, name)):
        if not trs:
            out.append((0, 0, 0, 0))
            continue
        assert trs == list(range(trs[0], trs[-1] + 1)) and tcs == list(range(tcs[0], tcs[-1] + 1)), "a rectangle"
        held = (r1 >> o) - (r0 >> o)
        lo, hi = trs[0] * TILE_ROWS >> o, min((trs[-1] + 1) * TILE_ROWS >> o, held)
        c_lo, c_hi = tcs[0] * TILE_COLS >> o, min((tcs[-1] + 1) * TILE_COLS >> o, W >> o)
        rows, gpr = max(0, hi - lo), max(0, -(-(c_hi - c_lo) // 4))
        out.append((lo, rows, c_lo, gpr) if rows and gpr else (0, 0, 0, 0))
    return out


def support_units(oracle, name):
    """The number of support units of one k_keep launch of the shape's context."""
    batch = SHAPES[name][4].get("batch", 1)
    groups = sum(rows * gpr for _, rows, _, gpr in group_rects(oracle, name))
    return -(-groups * batch // TAIL_GROUPS)


def tail_units(name):
    H, W, O, _, kw = SHAPES[name]
    r0, r1 = span(name)
    groups = sum(((r1 >> o) - (r0 >> o)) * -(-(W >> o) // 4) for o in range(FUSED, O))
    return -(-groups * kw.get("batch", 1) // TAIL_GROUPS)


def tiles(name):
    W, kw = SHAPES[name][1], SHAPES[name][4]
    r0, r1 = span(name)
    return -(-(r1 - r0) // TILE_ROWS) * -(-W // TILE_COLS) * kw.get("batch", 1)
