"""Time of gdp_match_descriptors (exact nearest / second-nearest descriptor matching on the i8 matrix
cores) against what a caller would do today with the records already on the device.

    python tools/match_bench.py [--n 4096] [--S 2] [--octaves 5] [--sizes 50:0,40:280615]
                                [--ratio 0.8] [--runs 20] [--warmup 3] [--torch-runs 0]

Workload: bench.py's config 2 (one 4096^2 image, S = 2, 5 octaves) after build_gaussian on the
synthetic image, then detect_extrema(contrast), refine_keypoints(0, 10), orient_keypoints and
describe_keypoints, once per entry CONTRAST:KEYPOINT_CAPACITY of --sizes (0: the default capacity):
the two list sizes of tools/describe_bench.py.  The described list is matched against itself — the
sweep's work does not depend on the values — with ratio 0.8, no cap, mutual off, and once more with
mutual on.  Each match (counter memset + norms + sweep + select) is timed with events on the launch
stream.

Baseline, same session, same stream, same timing: torch float32 on the same descriptors as float
tensors, na[:, None] + nb[None, :] - 2 A @ B.T and torch.topk(2, largest=False), in chunks of query
rows so that a distance block stays under 8 GiB.

Prints one JSON line per size with the medians and ranges, 2 * 128 * nq * nt / t in TOP/s for the
kernel path and its fraction of the dense i8 rate (--i8-peak-tops, default 5000)."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import __graft_entry__ as entry  # noqa: E402

BLOCK_BYTES = 8 << 30


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--S", type=int, default=2)
    ap.add_argument("--octaves", type=int, default=5)
    ap.add_argument("--sizes", default="50:0,40:280615")
    ap.add_argument("--ratio", type=float, default=0.8)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--torch-runs", type=int, default=0, help="0: the same as --runs")
    ap.add_argument("--i8-peak-tops", type=float, default=5000.0)
    a = ap.parse_args()
    if a.runs < 20:
        ap.error("--runs must be at least 20")

    import numpy as np
    import torch

    pkg = entry.load_package()
    stream = torch.cuda.Stream()

    def timed(call, runs):
        ms = []
        for i in range(a.warmup + runs):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record(stream)
            call()
            t1.record(stream)
            t1.synchronize()
            if i >= a.warmup:
                ms.append(t0.elapsed_time(t1))
        return ms

    def stats(name, ms):
        return {name + "_ms": round(statistics.median(ms), 5), name + "_ms_min": round(min(ms), 5), name + "_ms_max": round(max(ms), 5)}

    for size in a.sizes.split(","):
        contrast, capacity = size.split(":")
        contrast, capacity = float(contrast), int(capacity)
        with pkg.PyramidContext(a.n, a.n, S=a.S, octaves=a.octaves) as ctx:
            if capacity:
                ctx.set_keypoint_capacity(capacity)
            ctx.fill_synthetic(0x5EED, 0, stream=stream)
            ctx.build_gaussian(stream)
            ctx.detect_extrema(contrast, 0.0, stream=stream)
            ctx.refine_keypoints(0.0, 10.0, stream=stream)
            ctx.orient_keypoints(stream)
            ctx.describe_keypoints(stream)
            stream.synchronize()
            recs = ctx.described_keypoints(0)
            n = len(recs)
            assert n == recs.found, (n, recs.found)  # the capacity holds every record
            ctx.match_descriptors(ratio=a.ratio, stream=stream)  # the match object and its buffers exist before anything is timed
            stream.synchronize()
            layout = ctx.match_layout()
            match = timed(lambda: ctx.match_descriptors(ratio=a.ratio, stream=stream), a.runs)
            kept = ctx.match_count()
            mutual = timed(lambda: ctx.match_descriptors(ratio=a.ratio, mutual=True, stream=stream), a.runs)
            kept_mutual = ctx.match_count()

            with torch.cuda.stream(stream):
                A = torch.from_numpy(np.ascontiguousarray(recs["desc"]).astype(np.float32)).cuda()
                na = (A * A).sum(1)
            rows = max(1, min(n, BLOCK_BYTES // (4 * max(n, 1))))
            result = {}

            def baseline():
                with torch.cuda.stream(stream):
                    best = []
                    for i in range(0, n, rows):
                        d = na[i:i + rows, None] + na[None, :] - 2.0 * (A[i:i + rows] @ A.T)
                        best.append(torch.topk(d, 2, dim=1, largest=False))
                        del d
                    result["best"] = best

            ref = timed(baseline, a.torch_runs or a.runs)
            stream.synchronize()
            del result, A, na
            torch.cuda.empty_cache()
        med = statistics.median(match)
        tops = 2.0 * 128.0 * n * n / (med * 1e-3) / 1e12 if n else 0.0
        print(json.dumps({
            "op": "match_descriptors", "H": a.n, "W": a.n, "S": a.S, "octaves": a.octaves, "contrast": contrast,
            "keypoint_capacity": capacity or 65536, "nq": n, "nt": n, "ratio": a.ratio, "runs": a.runs,
            "match_capacity": layout[:2], "chunk_unit": layout[2], "train_chunks": layout[3], "query_chunks": layout[4],
            "kept": kept, "kept_mutual": kept_mutual, **stats("match", match), **stats("match_mutual", mutual),
            **stats("torch_f32", ref), "torch_rows_per_block": rows, "torch_runs": a.torch_runs or a.runs,
            "match_tops": round(tops, 2), "i8_peak_fraction": round(tops / a.i8_peak_tops, 4),
            "faster_than_torch": med < statistics.median(ref),
        }), flush=True)


if __name__ == "__main__":
    main()
