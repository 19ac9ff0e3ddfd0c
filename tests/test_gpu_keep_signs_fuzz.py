"""Model-based randomized sweep of k_keep's sign map (GDP_TUNE_KEEP_SIGNS, csrc/gdp_keep.inc).

The steady-state sweep's cases (tests/test_gpu_steady_fuzz.py: a sequence of builds on one context,
or one per row band, with one event before each build but the first) continued to FIVE builds, on
images that make the rule matter (tests/keep_signs_cases.py: most tile rows non-negative, the
others with a few negative pixels).  The CPU model of the map is carried per context: before and
after every build and after every event GDP_TUNE_SIGNS_KNOWN must equal the model's flag; after
every build every level of every image must equal the oracle's, uint32 views, +-0 included; after a
poison event the store map is exact in level S+2 too — the poison survives exactly on the words of
the row segments the model says ran no stores, in the (tile, octave) pairs k_keep stores from
registers.  The seed is fixed: a failure names its case.  Runs on an MI355X."""
import os
import time

import keep_signs_cases as ks
import numpy as np
import pytest
import steady_cases as sc
import test_gpu_steady_fuzz as base

pytestmark = pytest.mark.gpu

SCALE = max(1, int(os.environ.get("GDP_FUZZ_SCALE", "1")))
SEED = int(os.environ.get("GDP_FUZZ_SEED", "0"))
N_CASES = ks.DEFAULT_CASES * SCALE
CHUNKS = N_CASES // ks.CHUNK
_bits = base._bits


class _Run(base._Run):
    """The steady-state sweep's run of one case, with the model of the sign map beside it."""

    def __init__(self, pkg, oracle, case):
        self.pkg, self.oracle, self.case = pkg, oracle, case
        self.H, self.W, self.S, self.O, self.B = case["H"], case["W"], case["S"], case["Oeff"], case["B"]
        self.L = self.S + 3
        self.imgs = ks.images(case)
        self.wants = sc.oracle_pyramids(oracle, case, self.imgs)
        self.spans = sc.spans(case)
        self.ctxs, self.keep = [], []
        self.maps = [ks.SignMap(r1 - r0, self.W, self.B) for r0, r1 in self.spans]
        self.last = [(0, None)] * len(self.spans)  # (mode, stored) of every context's latest build
        self.stats = dict(mode2=0, skipped=0)

    def known(self, k, when):
        for ci, (ctx, m) in enumerate(zip(self.ctxs, self.maps)):
            got = ctx.tuning()["signs_known"]
            if got != int(m.known):
                self.fail(k, f"GDP_TUNE_SIGNS_KNOWN {when}", f"band {ci}: {got}, the model says {int(m.known)}")

    def event(self, k, ev):
        super().event(k, ev)
        if k and ev["kind"] in ("mutator", "centre", "bind_out", "unbind_out"):
            for m in self.maps:
                m.invalidate()
        self.known(k, f"after the event {ev['kind']}")

    def build(self, k, st):
        st = sc._snapshot(st, self.W)  # the rebuild after a poison event comes with clean = 0: a full build
        if st["clean"] == 0:
            for m in self.maps:
                m.invalidate()  # the event that cleared the flag (gdp_pyramid_written after a poison event)
        self.known(k, "before the build")
        super().build(k, st)
        for ci, (m, (r0, r1)) in enumerate(zip(self.maps, self.spans)):
            mode, stored, _ = m.build(st, [im[r0:r1] for im in self.imgs[k]])
            self.last[ci] = (mode, stored)
            if mode == 2:
                self.stats["mode2"] += 1
                self.stats["skipped"] += int((~stored).sum())
        self.known(k, "after the build")

    def check_store_map(self, k):
        """After a poison event: 0xFF survives in DoG levels 0..S+1 exactly on the words a kept
        build skips, and in level S+2 exactly on the words of the row segments that ran no stores;
        everything else is the oracle's."""
        for ci, ctx in enumerate(self.ctxs):
            dims = [ctx.level_dims(o) for o in range(self.O)]
            skipped = sc._skipped(self.oracle, self.H, self.W, self.O, self.S, dims)
            mode, stored = self.last[ci]
            masks = ks.fast_masks(self.oracle, self.case, self.spans[ci], dims) if mode == 2 else []
            for b in range(self.B):
                top = ks.unstored(masks, stored, b, dims) if mode == 2 else []
                for o in range(self.O):
                    for s in range(self.L):
                        g, w = _bits(ctx.level(b, o, s)), _bits(self.want_level(k, b, o, s, ctx))
                        where = f"band {ci}, (image, octave, scale) = {(b, o, s)}, sign mode {mode}"
                        if s == self.L - 1:
                            sk = top[o] if o < len(top) else np.zeros(g.shape, bool)
                        else:
                            sk = skipped[o]
                        assert sk.shape == g.shape and (w[sk] == 0).all(), (where, self.case)
                        made = np.argwhere(sk & (g != sc.POISON))
                        if made.size:
                            self.fail(k, "a store that this build does not owe was made",
                                      f"{where}, {len(made)} words, first (row, col) {made[:5].tolist()}: "
                                      f"{[hex(g[r, c]) for r, c in made[:5]]}")
                        bad = np.argwhere(~sk & (g != w))
                        if bad.size:
                            self.fail(k, "a store that this build owes is missing or wrong",
                                      f"{where}, {len(bad)} words, first (row, col) {bad[:5].tolist()}: "
                                      f"{[hex(g[r, c]) for r, c in bad[:5]]} vs {[hex(w[r, c]) for r, c in bad[:5]]}")


@pytest.mark.parametrize("chunk", range(CHUNKS))
def test_sign_map_sweep(pkg, oracle, chunk):
    """Cases [40 chunk, 40 chunk + 40) of the seeded sweep; a failure prints the case dict, the build
    index and (image, octave, scale, first differing words)."""
    cases = ks.cases(ks.DEFAULT_SEED + SEED, N_CASES)[chunk * ks.CHUNK:(chunk + 1) * ks.CHUNK]
    t0 = time.perf_counter()
    mode2 = skipped = 0
    for case in cases:
        run = _Run(pkg, oracle, case)
        try:
            run.run()
        except AssertionError:
            raise
        except Exception as e:  # a GdpError or HIP error: name the case it came from
            raise AssertionError(f"{type(e).__name__}: {e}\ncase = {case!r}") from e
        mode2 += run.stats["mode2"]
        skipped += run.stats["skipped"]
    print(f"sign-map sweep chunk {chunk}: {len(cases)} cases, {mode2} skipping builds, {skipped} row segments skipped, "
          f"{time.perf_counter() - t0:.2f} s")
