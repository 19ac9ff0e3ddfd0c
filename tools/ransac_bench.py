"""Time of gdp_fit_homography (RANSAC homography of a match list: four-point fits in float64, a dense
hypotheses x matches scoring sweep on the f32 VALU, selection, inlier compaction) against what a
caller would do today with the records already on the device.

    python tools/ransac_bench.py [--n 4096] [--S 2] [--octaves 5] [--sizes 50:0,40:280615]
                                 [--hypotheses 1024,4096] [--threshold 3.0] [--runs 20] [--warmup 3]

Workload: tools/match_bench.py's two lists (bench.py's config 2 after build_gaussian, detect, refine,
orient, describe, once per entry CONTRAST:KEYPOINT_CAPACITY of --sizes), each matched against itself
with the ratio test off, so the match list has one record per descriptor, every match is an inlier of
the identity and the sweep's work does not depend on the values.  Each fit (counter memset + fit +
score + select + inliers) is timed with events on the launch stream, H hypotheses each.

Baseline, same session, same stream, same timing: torch float32 on the four coordinates as tensors,
the H homographies SUPPLIED (the fit is excluded), step 5 as broadcast tensor operations over blocks
of hypotheses sized so that one H-block x n temporary stays under 8 GiB, sum for the counts, argmax.

Also reported, not gated: pairs per second; 21 separately rounded float operations per pair (12
products, 9 sums: the rule's, which is what the assembly issues, two pairs per packed instruction) as
a fraction of the f32 vector peak (--f32-peak-tflops, default 157.3, a rate that counts a fused
multiply-add as two — the rule forbids fusing, so half of it is the ceiling); and the time of the
same call on a caller's list of four records, where all that remains is k_ransac_fit and the launches.

Prints one JSON line per size and H."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import __graft_entry__ as entry  # noqa: E402

BLOCK_BYTES = 8 << 30
FLOPS_PER_PAIR = 21


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--S", type=int, default=2)
    ap.add_argument("--octaves", type=int, default=5)
    ap.add_argument("--sizes", default="50:0,40:280615")
    ap.add_argument("--hypotheses", default="1024,4096")
    ap.add_argument("--threshold", type=float, default=3.0)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--f32-peak-tflops", type=float, default=157.3)
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
            ctx.match_descriptors(ratio=0.0, stream=stream)
            stream.synchronize()
            recs = ctx.matches()
            n = len(recs)
            assert n == recs.found == ctx.described_count(0), (n, recs.found)  # one match per descriptor
            with torch.cuda.stream(stream):
                x, y, X, Y = (torch.from_numpy(np.ascontiguousarray(recs[f])).cuda()[None, :] for f in ("qx", "qy", "tx", "ty"))
            tt = float(np.float32(a.threshold) * np.float32(a.threshold))
            for H in (int(h) for h in a.hypotheses.split(",")):
                ctx.set_ransac_capacity(0, H)
                ctx.fit_homography(H, 1, a.threshold, stream=stream)  # the fit object and its buffers exist before anything is timed
                stream.synchronize()
                layout = ctx.ransac_layout()
                fit = timed(lambda: ctx.fit_homography(H, 1, a.threshold, stream=stream), a.runs)
                hyp, model, inliers = ctx.hypotheses(), ctx.homography(), ctx.inlier_count()

                with torch.cuda.stream(stream):
                    h = [torch.from_numpy(np.ascontiguousarray(hyp["h"][:, k])).cuda()[:, None] for k in range(9)]
                rows = max(1, min(H, BLOCK_BYTES // (4 * max(n, 1))))
                result = {}

                def baseline():
                    with torch.cuda.stream(stream):
                        counts = []
                        for i in range(0, H, rows):
                            g = [c[i:i + rows] for c in h]
                            u = (g[0] * x + g[1] * y) + g[2]
                            v = (g[3] * x + g[4] * y) + g[5]
                            w = (g[6] * x + g[7] * y) + g[8]
                            dx, dy = X * w - u, Y * w - v
                            counts.append(((w > 0) & (dx * dx + dy * dy <= tt * (w * w))).sum(1))
                            del u, v, w, dx, dy
                        counts = torch.cat(counts)
                        result["counts"], result["best"] = counts, torch.argmax(counts)

                ref = timed(baseline, a.runs)
                stream.synchronize()
                same = bool((result["counts"].cpu().numpy() == hyp["inliers"]).all())  # reported: torch may fuse or reorder
                del result, h
                torch.cuda.empty_cache()

                ctx.set_ransac_input(recs[:4])
                four = timed(lambda: ctx.fit_homography(H, 1, a.threshold, stream=stream), a.runs)
                ctx.set_ransac_input(None)

                med = statistics.median(fit)
                pairs = H * n / (med * 1e-3) if n else 0.0
                print(json.dumps({
                    "op": "fit_homography", "H": a.n, "W": a.n, "S": a.S, "octaves": a.octaves, "contrast": contrast,
                    "keypoint_capacity": capacity or 65536, "matches": n, "hypotheses": H, "threshold": a.threshold, "runs": a.runs,
                    "capacity": layout[0], "match_tile": layout[2], "hypothesis_tile": layout[3],
                    "model_hypothesis": int(model["hypothesis"]), "inliers": inliers,
                    **stats("fit", fit), **stats("torch_f32", ref), **stats("fit_of_four_records", four),
                    "torch_hypotheses_per_block": rows, "torch_counts_equal": same,
                    "pairs_per_s": round(pairs, 0), "f32_tflops": round(FLOPS_PER_PAIR * pairs / 1e12, 3),
                    "f32_peak_fraction": round(FLOPS_PER_PAIR * pairs / 1e12 / a.f32_peak_tflops, 4),
                    "speedup": round(statistics.median(ref) / med, 2), "ranges_overlap": not max(fit) < min(ref),
                    "faster_than_torch": max(fit) < min(ref),
                }), flush=True)


if __name__ == "__main__":
    main()
