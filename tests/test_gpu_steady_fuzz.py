"""Model-based randomized sweep of the steady-state build: kept rebuilds on random shapes and states.

Every case of tests/steady_cases.py is a SEQUENCE on one context (or one per row band): three builds
of three different images with one event before the second and one before the third — a download,
a detection, a refinement, a knob, the other input format, binding or unbinding the input or the
output, a pyramid writer, the other window centre, or 0xFF over the pyramid behind the library's
back.  Before every build GDP_TUNE_ZEROS_CLEAN must equal the model's flag, after it 1 (0 while a
caller's output is bound), and every level of every image must equal oracle.build_pyramid of that
build's image under the case's centre — uint32 views, +-0 included, no tolerance anywhere.  After a
poison event the store map is exact: the poison survives in DoG levels 0..S+1 exactly where a kept
build skips its stores and nowhere else.  After a refinement the keypoints and the refined records
equal the numpy oracles' on the oracle's pyramid.  The seed is fixed: a failure names its case.
Runs on an MI355X."""
import os
import time

import numpy as np
import pytest
import steady_cases as sc
from extrema_oracle import as_set, np_extrema
from refine_oracle import as_multiset, np_refine, records_from_set

pytestmark = pytest.mark.gpu

# as tests/test_gpu_fuzz.py: GDP_FUZZ_SCALE multiplies the case count (more chunks of the same
# size), GDP_FUZZ_SEED offsets the seed, for one-off long sweeps on hardware
SCALE = max(1, int(os.environ.get("GDP_FUZZ_SCALE", "1")))
SEED = int(os.environ.get("GDP_FUZZ_SEED", "0"))
N_CASES = sc.DEFAULT_CASES * SCALE
CHUNKS = N_CASES // sc.CHUNK


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


class _Run:
    """One case: its contexts (one per row band), the model's state and the oracle's pyramids."""

    def __init__(self, pkg, oracle, case):
        self.pkg, self.oracle, self.case = pkg, oracle, case
        self.H, self.W, self.S, self.O, self.B = case["H"], case["W"], case["S"], case["Oeff"], case["B"]
        self.L = self.S + 3
        self.imgs = sc.images(case)
        self.wants = sc.oracle_pyramids(oracle, case, self.imgs)
        self.spans = sc.spans(case)
        self.ctxs, self.keep = [], []

    def fail(self, build, what, detail=None):
        raise AssertionError(f"{what}: build {build}, {detail}\ncase = {self.case!r}")

    # -------------------------------------------------------------------------------- the sequence
    def run(self):
        c, st = self.case, self.case["builds"][0]
        try:
            for r0, r1 in self.spans:
                ctx = self.pkg.PyramidContext(self.H, self.W, S=self.S, octaves=c["O"], batch=self.B, row_begin=r0, row_end=r1,
                                              input_format=st["fmt"])
                self.ctxs.append(ctx)
                assert ctx.O == self.O, c
                assert [ctx.level_dims(o) for o in range(self.O)] == sc.band_dims(c, (r0, r1)), c
                ctx.set_tuning(**{k: st[k] for k in sc.KNOBS})
                ctx.set_window_centre(st["centre"])
            for k, st in enumerate(c["builds"]):
                ev = c["events"][k - 1] if k else dict(kind="none")
                self.event(k, ev)
                self.build(k, st)
                if ev["kind"] == "poison":
                    self.check_store_map(k)
                    for ctx in self.ctxs:
                        ctx.pyramid_written(-1)
                        if ctx.tuning()["zeros_clean"] != 0:
                            self.fail(k, "pyramid_written left the flag set")
                    self.build(k, dict(st, clean=0))  # restores every word
                self.check(k)
        finally:
            for ctx in self.ctxs:
                ctx.close()

    def build(self, k, st):
        import torch

        for ctx, (r0, r1) in zip(self.ctxs, self.spans):
            got = ctx.tuning()["zeros_clean"]
            if got != st["clean"]:
                self.fail(k, "GDP_TUNE_ZEROS_CLEAN before the build", f"{got}, the model says {st['clean']}")
            per = self.imgs[k]
            if st["in_bound"]:
                host = np.zeros((self.B, self.H, st["pitch"]), per[0].dtype)
                for b in range(self.B):
                    host[b, :, :self.W] = per[b]
                dev = torch.from_numpy(host).cuda()
                torch.cuda.synchronize()
                ctx.bind_device_input(dev.data_ptr(), st["pitch"], self.H * st["pitch"], keepalive=dev)
            else:
                for b in range(self.B):
                    ctx.set_input(np.ascontiguousarray(per[b][r0:r1]), b)
            if ctx.tuning()["zeros_clean"] != st["clean"]:
                self.fail(k, "a new input changed GDP_TUNE_ZEROS_CLEAN")
            ctx.build()
            after = ctx.tuning()["zeros_clean"]
            if after != (0 if st["out_bound"] else 1):
                self.fail(k, "GDP_TUNE_ZEROS_CLEAN after the build", f"{after}, output bound: {st['out_bound']}")
        for ctx in self.ctxs:
            ctx.sync()

    # -------------------------------------------------------------------------------- the checks
    def want_level(self, k, b, o, s, ctx):
        rows, cols, first = ctx.level_dims(o)
        off = self.oracle.level_offset(self.H, self.W, self.S, o, s)
        w = self.wants[k][b][off:off + (self.H >> o) * (self.W >> o)].reshape(self.H >> o, self.W >> o)
        return w[first:first + rows]

    def check(self, k):
        """Every level of every image, word for word."""
        for ci, ctx in enumerate(self.ctxs):
            for b in range(self.B):
                if len(self.ctxs) == 1 and np.array_equal(_bits(ctx.pyramid(b)), _bits(self.wants[k][b])):
                    continue  # the packed download of a whole image is the oracle's layout
                for o in range(self.O):
                    for s in range(self.L):
                        g, w = _bits(ctx.level(b, o, s)).ravel(), _bits(self.want_level(k, b, o, s, ctx)).ravel()
                        where = f"band {ci}, (image, octave, scale) = {(b, o, s)}"
                        if g.shape != w.shape:
                            self.fail(k, "a level has another shape than the oracle's", f"{where}: {g.shape} vs {w.shape}")
                        bad = np.flatnonzero(g != w)
                        if bad.size:
                            self.fail(k, "the pyramid differs from the oracle's",
                                      f"{where}, {bad.size} words of {g.size}, first at {bad[:5]}: {g[bad[:5]]} vs {w[bad[:5]]}")
                if len(self.ctxs) == 1:
                    self.fail(k, "gdp_download_pyramid differs from the levels it packs", f"image {b}")

    def check_store_map(self, k):
        """After a poison event: 0xFF survives in DoG levels 0..S+1 exactly on the skipped words;
        everything else, and all of level S+2, is the oracle's."""
        for ci, ctx in enumerate(self.ctxs):
            skipped = sc._skipped(self.oracle, self.H, self.W, self.O, self.S, [ctx.level_dims(o) for o in range(self.O)])
            for b in range(self.B):
                for o in range(self.O):
                    for s in range(self.L):
                        g, w = _bits(ctx.level(b, o, s)), _bits(self.want_level(k, b, o, s, ctx))
                        where = f"band {ci}, (image, octave, scale) = {(b, o, s)}"
                        if s == self.L - 1:
                            sk = np.zeros(g.shape, bool)
                        else:
                            sk = skipped[o]
                            assert sk.shape == g.shape and (w[sk] == 0).all(), (where, self.case)
                            made = np.argwhere(sk & (g != sc.POISON))
                            if made.size:
                                self.fail(k, "a store that a kept build skips was made",
                                          f"{where}, {len(made)} words, first (row, col) {made[:5].tolist()}: "
                                          f"{[hex(g[r, c]) for r, c in made[:5]]}")
                        bad = np.argwhere(~sk & (g != w))
                        if bad.size:
                            self.fail(k, "a store that a kept build owes is missing or wrong",
                                      f"{where}, {len(bad)} words, first (row, col) {bad[:5].tolist()}: "
                                      f"{[hex(g[r, c]) for r, c in bad[:5]]} vs {[hex(w[r, c]) for r, c in bad[:5]]}")

    # -------------------------------------------------------------------------------- the events
    def event(self, k, ev):
        import torch

        kind = ev["kind"]
        for ci, ctx in enumerate(self.ctxs):
            if kind == "reader":
                b, o, s = int(k % self.B), (k + ci) % self.O, k % self.L
                if ev["what"] == "level":
                    got, want = ctx.level(b, o, s), self.want_level(k - 1, b, o, s, ctx)
                    if not np.array_equal(_bits(got), _bits(want)):
                        self.fail(k, "gdp_download_level after the build", (b, o, s))
                elif ev["what"] == "pyramid":
                    want = np.concatenate([self.want_level(k - 1, b, oo, ss, ctx).ravel()
                                           for oo in range(self.O) for ss in range(self.L)])
                    got = ctx.pyramid(b)
                    if got.shape != want.shape or not np.array_equal(_bits(got), _bits(want)):
                        self.fail(k, "gdp_download_pyramid after the build", f"band {ci}, image {b}")
                else:
                    ctx.detect_extrema()
                    if ev["what"] == "keypoints":
                        found, _ = np_extrema(self.wants[k - 1][b], self.H, self.W, self.S, self.O)
                        if as_set(ctx.keypoints(b)) != found:
                            self.fail(k, "gdp_detect_extrema on the build's output", f"image {b}")
            elif kind == "refine":
                ctx.detect_extrema(ev["contrast"], ev["edge_ratio"])
                ctx.refine_keypoints(ev["contrast"], ev["edge_ratio"])  # the same stream, nothing in between
                for b in range(self.B):
                    pyr = self.wants[k - 1][b]  # the oracle's pyramid of the current image
                    found, _ = np_extrema(pyr, self.H, self.W, self.S, self.O, ev["contrast"], ev["edge_ratio"])
                    if as_set(ctx.keypoints(b)) != found:
                        self.fail(k, "gdp_detect_extrema on the build's output", f"image {b}, {len(found)} expected")
                    kept, _ = np_refine(pyr, self.H, self.W, self.S, self.O, records_from_set(found), ev["contrast"],
                                        ev["edge_ratio"])
                    got = ctx.refined_keypoints(b)
                    if ctx.refined_count(b) != len(got) or as_multiset(got) != kept:
                        self.fail(k, "gdp_refine_keypoints on the build's output",
                                  f"image {b}, {len(got)} records, {len(kept)} expected of {len(found)} keypoints")
            elif kind == "knob":
                ctx.set_tuning(**ev["set"])
            elif kind == "format":
                ctx.set_input_format(ev["fmt"])
            elif kind == "unbind_in":
                ctx.unbind_device_input()
            elif kind == "mutator":
                what = ev["what"]
                if what == "upload_level":
                    ctx.upload_level(ev["b"], ev["o"], ev["s"], np.full(ctx.level_dims(ev["o"])[:2], np.nan, np.float32))
                elif what == "generate_dog":
                    ctx.generate_dog()
                elif what == "gauss_range":
                    ctx.gauss_range(0, self.O)
                elif what == "init":
                    ctx.init()
                else:
                    ctx.pyramid_written(ev["b"])
            elif kind == "centre":
                ctx.set_window_centre(ev["centre"])
            elif kind == "bind_out":
                buf = torch.full((ctx.pyramid_bytes() // 4,), float("nan"), device="cuda")
                torch.cuda.synchronize()
                ctx.bind_device_output(buf.data_ptr(), ctx.pyramid_bytes(), keepalive=buf)
            elif kind == "unbind_out":
                ctx.unbind_device_output()
            elif kind == "poison":
                sc._poison(ctx)
            # "none", and "bind_in" (the build binds the new image's buffer): nothing to do here
            if k and ctx.tuning()["zeros_clean"] != ev["clean"]:
                self.fail(k, f"GDP_TUNE_ZEROS_CLEAN after the event {kind}",
                          f"{ctx.tuning()['zeros_clean']}, the model says {ev['clean']}")


@pytest.mark.parametrize("chunk", range(CHUNKS))
def test_steady_state_sweep(pkg, oracle, chunk):
    """Cases [40 chunk, 40 chunk + 40) of the seeded sweep; a failure prints the case dict, the build
    index and (image, octave, scale, first differing words)."""
    cases = sc.cases(sc.DEFAULT_SEED + SEED, N_CASES)[chunk * sc.CHUNK:(chunk + 1) * sc.CHUNK]
    t0 = time.perf_counter()
    kept = k_keep = 0
    for case in cases:
        try:
            _Run(pkg, oracle, case).run()
        except AssertionError:
            raise
        except Exception as e:  # a GdpError or HIP error: name the case it came from
            raise AssertionError(f"{type(e).__name__}: {e}\ncase = {case!r}") from e
        kept += sum(st["kept"] for st in case["builds"])
        k_keep += sum(st["k_keep"] for st in case["builds"])
    print(f"steady-state sweep chunk {chunk}: {len(cases)} cases, {kept} kept builds ({k_keep} by k_keep), "
          f"{time.perf_counter() - t0:.2f} s")
