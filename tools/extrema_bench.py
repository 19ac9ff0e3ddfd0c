"""Kernel time of gdp_detect_extrema (scale-space extrema on the device-resident DoG pyramid).

    python tools/extrema_bench.py [--n 4096] [--S 2] [--octaves 5] [--contrast 50] [--edge-ratio 0]
                                  [--runs 40] [--warmup 5] [--sweep]

Workload: bench.py's config 2 (one 4096^2 image, S = 2, 5 octaves) after build_gaussian on the
synthetic image.  Like bench.py, the detection rotates over enough independent contexts to exceed
2 GiB of pyramid, so every launch reads its levels from HBM, not from a cache the previous launch
filled.  Each detect_extrema (counter memset + one kernel) is timed with events on the launch
stream; prints one JSON line with the median ms, the algorithmic read bytes 4 (S+2) sum_o rows_o
cols_o, their share of 8 TB/s and the keypoints found.  --sweep first prints `found` for a ladder
of contrast thresholds (to pick one that leaves a few thousand keypoints: 50 on the synthetic
image), each with the time of one warm launch."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import __graft_entry__ as entry  # noqa: E402

ROTATE_BYTES = 2 << 30
PEAK_BYTES_PER_S = 8e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--S", type=int, default=2)
    ap.add_argument("--octaves", type=int, default=5)
    ap.add_argument("--contrast", type=float, default=50.0)
    ap.add_argument("--edge-ratio", type=float, default=0.0)
    ap.add_argument("--runs", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sweep", action="store_true")
    a = ap.parse_args()
    if a.runs < 20:
        ap.error("--runs must be at least 20")

    import torch

    pkg = entry.load_package()
    first = pkg.PyramidContext(a.n, a.n, S=a.S, octaves=a.octaves)
    rotate = max(1, -(-ROTATE_BYTES // first.pyramid_bytes()))
    ctxs = [first] + [pkg.PyramidContext(a.n, a.n, S=a.S, octaves=a.octaves) for _ in range(rotate - 1)]
    stream = torch.cuda.Stream()
    for c in ctxs:  # identical images at different addresses
        c.fill_synthetic(0x5EED, 0, stream=stream)
        c.build_gaussian(stream)
    stream.synchronize()
    read_bytes = 4 * (a.S + 2) * sum(first.level_dims(o)[0] * first.level_dims(o)[1] for o in range(first.O))

    if a.sweep:
        for thr in (0.0, 1.0, 2.0, 5.0, 10.0, 20.0, 30.0, 40.0, 50.0, 60.0, 80.0, 100.0):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            for _ in range(2):  # the second, warm launch is the one reported (one context: cache-assisted)
                t0.record(stream)
                first.detect_extrema(thr, a.edge_ratio, stream=stream)
                t1.record(stream)
                t1.synchronize()
            print(json.dumps({"sweep_contrast": thr, "found": first.keypoint_count(0),
                              "ms_one_context": round(t0.elapsed_time(t1), 5)}), flush=True)

    ms = []
    for i in range(a.warmup + a.runs):
        c = ctxs[i % rotate]
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(stream)
        c.detect_extrema(a.contrast, a.edge_ratio, stream=stream)
        t1.record(stream)
        t1.synchronize()
        if i >= a.warmup:
            ms.append(t0.elapsed_time(t1))
    found = [c.keypoint_count(0) for c in ctxs]
    assert len(set(found)) == 1, found  # the same image everywhere
    med = statistics.median(ms)
    print(json.dumps({
        "op": "detect_extrema", "H": a.n, "W": a.n, "S": a.S, "octaves": first.O, "contrast": a.contrast,
        "edge_ratio": a.edge_ratio, "rotate": rotate, "pyramid_bytes": first.pyramid_bytes(), "runs": a.runs,
        "ms": round(med, 5), "ms_min": round(min(ms), 5), "ms_max": round(max(ms), 5), "read_bytes": read_bytes,
        "read_TBps": round(read_bytes / (med * 1e-3) / 1e12, 3),
        "pct_of_8TBps": round(100.0 * read_bytes / (med * 1e-3) / PEAK_BYTES_PER_S, 1), "found": found[0],
    }), flush=True)
    for c in ctxs:
        c.close()


if __name__ == "__main__":
    main()
