"""Time of gdp_refit_homography (least-squares refit of the RANSAC homography over its inliers: exact
128-bit integer moments, one 8 x 8 solve in float64, rescoring of the model and the candidate, the
decision, inlier compaction) against what a caller would do today with the records already on the
device.

    python tools/refit_bench.py [--n 4096] [--S 2] [--octaves 5] [--sizes 50:0,40:280615]
                                [--hypotheses 1024] [--threshold 3.0] [--runs 20] [--warmup 3]

Workload: tools/ransac_bench.py's two lists (bench.py's config 2 after build_gaussian, detect, refine,
orient, describe, once per entry CONTRAST:KEYPOINT_CAPACITY of --sizes), each matched against itself
with the ratio test off, so every match is an inlier of the identity and the inlier list is the whole
list.  Before every timed call a fit of --hypotheses hypotheses is launched on the same stream (not
timed), so each refit starts from the RANSAC winner; events on the launch stream surround one
refit_homography(rounds=1): one memset and seven launches.

Baseline, same session, same stream, same timing: torch float64 on the four inlier coordinates as
tensors: the 2n x 8 system of the inhomogeneous DLT, torch.linalg.lstsq, then step 5 of the fit rule
for the one matrix as broadcast float32 tensor operations and a sum.  Also reported, not gated: the
same with the 8 x 8 normal equations and torch.linalg.solve in place of lstsq (what a caller who
knows the system is well conditioned would write); the whole refit call on a caller's list of four
records, which is the fixed cost of the launches; and the refit model's largest difference from the
torch solution.

Prints one JSON line per size."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import __graft_entry__ as entry  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--S", type=int, default=2)
    ap.add_argument("--octaves", type=int, default=5)
    ap.add_argument("--sizes", default="50:0,40:280615")
    ap.add_argument("--hypotheses", type=int, default=1024)
    ap.add_argument("--threshold", type=float, default=3.0)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    if a.runs < 20:
        ap.error("--runs must be at least 20")

    import numpy as np
    import torch

    pkg = entry.load_package()
    stream = torch.cuda.Stream()

    def timed(call, runs, before=lambda: None):
        ms = []
        for i in range(a.warmup + runs):
            before()
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
            n = ctx.match_count()
            ctx.set_ransac_capacity(0, a.hypotheses)

            def fit():
                ctx.fit_homography(a.hypotheses, 1, a.threshold, stream=stream)

            fit()
            ctx.refit_homography(1, a.threshold, stream=stream)  # the refit's buffers exist before anything is timed
            stream.synchronize()
            refit = timed(lambda: ctx.refit_homography(1, a.threshold, stream=stream), a.runs, fit)
            model, rec, inliers = ctx.homography(), ctx.refit_record(), ctx.inlier_count()
            fit()
            stream.synchronize()
            L = ctx.inliers()  # the RANSAC winner's inliers: what the baseline solves on
            with torch.cuda.stream(stream):
                x, y, X, Y = (torch.from_numpy(np.ascontiguousarray(L[f]).astype(np.float64)).cuda() for f in ("qx", "qy", "tx", "ty"))
                M = ctx.matches()
                mx, my, mX, mY = (torch.from_numpy(np.ascontiguousarray(M[f])).cuda() for f in ("qx", "qy", "tx", "ty"))
            tt = float(np.float32(a.threshold) * np.float32(a.threshold))
            result = {}

            def system():
                one, zero = torch.ones_like(x), torch.zeros_like(x)
                A = torch.cat([torch.stack([x, y, one, zero, zero, zero, -X * x, -X * y], 1),
                               torch.stack([zero, zero, zero, x, y, one, -Y * x, -Y * y], 1)])
                return A, torch.cat([X, Y])

            def rescore(g):
                h = torch.cat([g, torch.ones(1, dtype=g.dtype, device=g.device)]).float()
                u = (h[0] * mx + h[1] * my) + h[2]
                v = (h[3] * mx + h[4] * my) + h[5]
                w = (h[6] * mx + h[7] * my) + h[8]
                dx, dy = mX * w - u, mY * w - v
                result["h"], result["count"] = h, ((w > 0) & (dx * dx + dy * dy <= tt * (w * w))).sum()

            def baseline_lstsq():
                with torch.cuda.stream(stream):
                    A, b = system()
                    rescore(torch.linalg.lstsq(A, b[:, None]).solution[:, 0])

            def baseline_normal():
                with torch.cuda.stream(stream):
                    A, b = system()
                    rescore(torch.linalg.solve(A.T @ A, A.T @ b))

            ref = timed(baseline_lstsq, a.runs)
            stream.synchronize()
            h_ref, count_ref = result["h"].double().cpu().numpy(), int(result["count"])
            normal = timed(baseline_normal, a.runs)
            stream.synchronize()
            del x, y, X, Y, mx, my, mX, mY
            torch.cuda.empty_cache()

            ctx.set_ransac_input(M[:4])
            four = timed(lambda: ctx.refit_homography(1, a.threshold, stream=stream), a.runs, fit)
            ctx.set_ransac_input(None)

            h = np.asarray(model["h"], np.float64)
            med = statistics.median(refit)
            print(json.dumps({
                "op": "refit_homography", "H": a.n, "W": a.n, "S": a.S, "octaves": a.octaves, "contrast": contrast,
                "keypoint_capacity": capacity or 65536, "matches": n, "hypotheses": a.hypotheses, "threshold": a.threshold, "runs": a.runs,
                "capacity": ctx.ransac_layout()[0], "inliers_of_the_fit": len(L), "inliers": inliers, "status": int(rec["status"]),
                "used": int(rec["used"]), "kq": int(rec["kq"]), "kt": int(rec["kt"]),
                **stats("refit", refit), **stats("torch_f64_lstsq", ref), **stats("torch_f64_normal_equations", normal),
                **stats("refit_of_four_records", four),
                "torch_count": count_ref, "max_abs_difference_from_torch": float(np.abs(h / h[8] - h_ref / h_ref[8]).max()),
                "speedup": round(statistics.median(ref) / med, 2), "speedup_over_normal_equations": round(statistics.median(normal) / med, 2),
                "ranges_overlap": not max(refit) < min(ref), "faster_than_torch": max(refit) < min(ref),
            }), flush=True)


if __name__ == "__main__":
    main()
