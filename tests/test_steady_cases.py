"""CPU checks of the steady-state sweep's case generator (tests/steady_cases.py): a sweep proves
nothing if its cases avoid the hard paths, so the default seed's cases must reach every one of
them.  These are conditions on the draw, not measurements: the 16 x 256 tile seams, grid and tail
of k_keep (csrc/gdp_keep.inc), its fast and slow path per (tile, octave), every way a context is not
eligible for it, every event kind, and the format switch in front of a kept build."""
import collections
import copy

import numpy as np
import pytest
import steady_cases as sc

MIN_CASES = 5


@pytest.fixture(scope="module")
def cases():
    return sc.cases(sc.DEFAULT_SEED, sc.DEFAULT_CASES)


def _kept_builds(case):
    """(event before it, model state) of the builds after the first."""
    return list(zip(case["events"], case["builds"][1:]))


def _k_keep(case):
    return any(st["k_keep"] for _, st in _kept_builds(case))


def test_draw_is_deterministic_and_pure(cases):
    again = sc.cases(sc.DEFAULT_SEED, sc.DEFAULT_CASES)
    assert again == cases
    assert sc.cases(sc.DEFAULT_SEED + 1, 8) != cases[:8]
    before = copy.deepcopy(cases[3])
    a, b = sc.images(cases[3]), sc.images(cases[3])
    assert cases[3] == before
    assert all(np.array_equal(x, y) and x.dtype == y.dtype for pa, pb in zip(a, b) for x, y in zip(pa, pb))


def test_geometry_ranges_and_the_model_of_the_flag(cases):
    for c in cases:
        H, W = c["H"], c["W"]
        assert 1 <= H <= 320 and 1 <= W <= 2100 and (W <= 644 or (H <= 64 and W % 4 == 0)), c
        assert 0 <= c["S"] <= 4 and 1 <= c["B"] <= 3 and 1 <= c["Oeff"] <= int(np.log2(min(H, W))) + 1, c
        assert len(c["builds"]) == sc.N_BUILDS and len(c["events"]) == sc.N_BUILDS - 1
        assert c["builds"][0]["clean"] == 0  # the first build of a context stores every byte
        for ev, st in _kept_builds(c):
            assert ev["kind"] in sc.EVENT_KINDS and ev["clean"] == st["clean"], c
            if st["out_bound"]:
                assert st["clean"] == 0, c  # never kept while a caller's output is bound
            if ev["kind"] in ("mutator", "centre", "bind_out", "unbind_out"):
                assert ev["clean"] == 0, c
            if ev["kind"] == "poison":
                assert ev["clean"] == 1, c
            if ev["kind"] == "refine":
                assert c["bands"] is None, c
        if c["bands"]:
            align = 1 << (max(c["Oeff"], 5) - 1)
            assert c["B"] == 1 and c["bands"][0][0] == 0 and c["bands"][-1][1] == H
            assert all(a < b and a % align == 0 for a, b in c["bands"])
            assert all(p[1] == q[0] for p, q in zip(c["bands"], c["bands"][1:]))


def test_images_change_sign_between_builds(cases):
    """Image k+1 has the opposite sign of image k over large areas; every int32 image has zeros and
    INT32_MIN pixels of its own."""
    seen = 0
    for c in cases[:40]:
        imgs = sc.images(c)
        for k in range(sc.N_BUILDS):
            for b in range(c["B"]):
                im = imgs[k][b]
                assert im.shape == (c["H"], c["W"])
                assert im.dtype == (np.uint8 if c["builds"][k]["fmt"] == "u8" else np.int32)
                if im.dtype == np.int32:
                    assert (im == 0).any() and (im == sc.INT32_MIN).any()
                if k and im.dtype == np.int32 and imgs[k - 1][b].dtype == np.int32 and im.size >= 64:
                    flipped = (np.sign(im.astype(np.int64)) == -np.sign(imgs[k - 1][b].astype(np.int64))).mean()
                    assert flipped > 0.8, (c, k, b, flipped)
                    seen += 1
    assert seen >= 40


def test_most_cases_skip_more_than_a_quarter_of_their_dog_words(cases, oracle):
    frac = [sc.skipped_fraction(oracle, c) for c in cases]
    assert sum(f > 0.25 for f in frac) >= 0.8 * len(cases), sorted(frac)[:40]


def test_the_default_seed_reaches_every_hard_path(cases, oracle):
    def kernel(v):
        return lambda c: any(st["k_keep"] and st["keep_kernel"] == v for _, st in _kept_builds(c))

    conditions = {
        "k_keep with keep_kernel 1": kernel(1),
        "k_keep with keep_kernel 2": kernel(2),
        "two or more tile columns": lambda c: _k_keep(c) and c["W"] > 256,
        "a last tile column of one group": lambda c: _k_keep(c) and c["W"] % 256 == 4,
        "a partial last tile row": lambda c: _k_keep(c) and c["H"] % 16 != 0,
        "less than one tile row": lambda c: _k_keep(c) and c["H"] < 16,
        "fewer octaves than the fused five": lambda c: _k_keep(c) and c["Oeff"] < 5,
        "tail octaves": lambda c: _k_keep(c) and c["Oeff"] > 5,
        "a grid cap below the unit count": lambda c: any(st["k_keep"] and 0 < st["grid"] < sc.keep_units(c)
                                                         for _, st in _kept_builds(c)),
        "nontemporal = 0": lambda c: any(st["k_keep"] and st["nontemporal"] == 0 for _, st in _kept_builds(c)),
        "batch > 1": lambda c: _k_keep(c) and c["B"] > 1,
        "a band with row_begin != 0": lambda c: c["bands"] is not None and any(r0 for r0, _ in c["bands"]),
        "a k_keep band with row_begin != 0": lambda c: c["bands"] is not None and _k_keep(c),
        "an octave-3 or octave-4 clean tile": lambda c: _k_keep(c) and sum(sc.clean_tiles(oracle, c)[3:]) > 0,
        "not eligible by width": lambda c: c["W"] % 4 != 0 and any(st["kept"] and st["keep_kernel"] > 0
                                                                   for _, st in _kept_builds(c)),
        "not eligible by pitch": lambda c: c["W"] % 4 == 0 and any(st["kept"] and st["keep_kernel"] > 0 and not st["eligible"]
                                                                   for _, st in _kept_builds(c)),
        "int32 -> uint8 directly before a k_keep build": lambda c: any(
            ev["kind"] == "format" and ev["fmt"] == "u8" and st["k_keep"] for ev, st in _kept_builds(c)),
        "uint8 -> int32 directly before a k_keep build": lambda c: any(
            ev["kind"] == "format" and ev["fmt"] == "i32" and st["k_keep"] for ev, st in _kept_builds(c)),
        "a kept build on k_build's keep path": lambda c: any(st["kept"] and not st["k_keep"] for _, st in _kept_builds(c)),
        "S = 2 (the L == 5 instances) kept": lambda c: c["S"] == 2 and any(st["kept"] for _, st in _kept_builds(c)),
    }
    counts = {name: sum(bool(f(c)) for c in cases) for name, f in conditions.items()}
    assert all(n >= MIN_CASES for n in counts.values()), counts
    events = collections.Counter(ev["kind"] for c in cases for ev in c["events"])
    assert all(events[k] >= MIN_CASES for k in sc.EVENT_KINDS), events
    assert {ev["what"] for c in cases for ev in c["events"] if ev["kind"] == "mutator"} == set(sc.MUTATORS)
    assert {ev["what"] for c in cases for ev in c["events"] if ev["kind"] == "reader"} == set(sc.READERS)


def test_every_oracle_pyramid_builds_here(cases, oracle):
    """The sweep's expected values: every build of every case, under that build's centre."""
    for c in cases:
        wants = sc.oracle_pyramids(oracle, c)
        assert len(wants) == sc.N_BUILDS
        for per in wants:
            assert len(per) == c["B"]
            for w in per:
                assert w.dtype == np.float32 and w.size == oracle.pyramid_floats(c["H"], c["W"], c["S"], c["Oeff"])
