"""Kernel time of the steady-state build (k_keep) by the sign of its input (GDP_TUNE_KEEP_SIGNS).

    python tools/keep_signs_bench.py [--n 4096] [--batch 1] [--S 2] [--octaves 5] [--runs 40] [--warmup 10]
                                     [--keep-kernel N] [--keep-signs N] [--contexts 5]

Workload: bench.py's config 2 (one 4096^2 int32 image, S = 2, 5 octaves), five contexts in rotation
as there, each build timed with events on the launch stream after every context has reached its
steady state (two builds each at least).  Three inputs, one JSON line each with the median of
--runs launches:
  nonneg        every pixel in 0..255: no row owes a level-S+2 store (the case the sign map is for)
  negative      every pixel negative: every row stores, the ballot and the flag load are pure overhead
  one_per_row   one negative pixel per 16-row tile row: that row's segments store in one tile column
and a fourth line, `establish`: on the non-negative input, gdp_pyramid_written, a full build and
then the TIMED build — the first steady-state build after an invalidation, which makes every store
and (with the knob on) writes the map.
`shape` is the k_keep shape the timed launches ran: GDP_TUNE_KEEP_SIGNS_KERNEL for a launch that
skips by the map, GDP_TUNE_KEEP_KERNEL for every launch that makes the stores.
--keep-signs / --keep-kernel are left at the library's defaults unless given, so the same file
times a library without the knob."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import __graft_entry__ as entry  # noqa: E402


def inputs(n, batch):
    rng = np.random.default_rng(0x5EED)
    base = rng.integers(0, 256, size=(n, n), dtype=np.int64).astype(np.int32)
    one = base.copy()
    rows = np.arange(0, n, 16) + rng.integers(0, 16, size=-(-n // 16))
    one[np.minimum(rows, n - 1), rng.integers(0, n, size=rows.size)] = -1
    return {"nonneg": base, "negative": -base - 1, "one_per_row": one}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--S", type=int, default=2)
    ap.add_argument("--octaves", type=int, default=5)
    ap.add_argument("--runs", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--contexts", type=int, default=5)
    ap.add_argument("--keep-kernel", type=int, default=None)
    ap.add_argument("--keep-signs", type=int, default=None)
    a = ap.parse_args()
    if a.runs < 20:
        ap.error("--runs must be at least 20")

    import torch

    pkg = entry.load_package()
    ctxs = [pkg.PyramidContext(a.n, a.n, S=a.S, octaves=a.octaves, batch=a.batch) for _ in range(a.contexts)]
    knobs = {k: v for k, v in (("keep_kernel", a.keep_kernel), ("keep_signs", a.keep_signs)) if v is not None}
    for c in ctxs:
        c.set_tuning(**knobs)
    stream = torch.cuda.Stream()

    def report(name, ms, establishing):
        sums = {c.checksum(0) for c in ctxs}
        assert len(sums) == 1, sums  # the same image everywhere
        tun = ctxs[0].tuning()
        skipping = tun.get("keep_signs") and tun.get("signs_known") and not establishing
        med = statistics.median(ms)
        print(json.dumps({
            "op": "build (steady state)", "input": name, "H": a.n, "W": a.n, "batch": a.batch, "S": a.S, "octaves": ctxs[0].O,
            "contexts": a.contexts, "runs": a.runs, "keep_kernel": tun.get("keep_kernel"), "keep_signs": tun.get("keep_signs"),
            "signs_known": tun.get("signs_known"), "shape": tun.get("keep_signs_kernel") if skipping else tun.get("keep_kernel"),
            "ms": round(med, 5), "ms_min": round(min(ms), 5),
            "ms_max": round(max(ms), 5), "input_bytes": 4 * a.n * a.n * a.batch,
            "input_TBps": round(4 * a.n * a.n * a.batch / (med * 1e-3) / 1e12, 3), "checksum": sums.pop(),
        }), flush=True)

    all_inputs = inputs(a.n, a.batch)
    for name, img in all_inputs.items():
        for c in ctxs:
            for b in range(a.batch):
                c.set_input(img, b)
            c.sync()
        ms = []
        for i in range(max(a.warmup, 2 * a.contexts) + a.runs):
            c = ctxs[i % a.contexts]
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record(stream)
            c.build(stream)
            t1.record(stream)
            t1.synchronize()
            ms.append(t0.elapsed_time(t1))
        ms = ms[-a.runs:]
        report(name, ms, False)
    # the first steady-state build after an invalidation
    for c in ctxs:
        for b in range(a.batch):
            c.set_input(all_inputs["nonneg"], b)
        c.sync()
    ms = []
    for i in range(a.contexts + a.runs):
        c = ctxs[i % a.contexts]
        c.pyramid_written(-1)
        c.build(stream)  # the full build
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(stream)
        c.build(stream)
        t1.record(stream)
        t1.synchronize()
        ms.append(t0.elapsed_time(t1))
    report("establish", ms[-a.runs:], True)
    for c in ctxs:
        c.close()


if __name__ == "__main__":
    main()
