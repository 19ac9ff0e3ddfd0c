"""Kernel time of gdp_describe_keypoints (SIFT descriptors of the oriented list on the device).

    python tools/describe_bench.py [--n 4096] [--S 2] [--octaves 5] [--contrast 50] [--edge-ratio 0]
                                   [--refine-contrast 0] [--refine-edge-ratio 10] [--capacity 0]
                                   [--runs 40] [--warmup 5]

Workload: bench.py's config 2 (one 4096^2 image, S = 2, 5 octaves) after build_gaussian on the
synthetic image, then detect_extrema(contrast, edge-ratio), refine_keypoints(refine-contrast,
refine-edge-ratio) and orient_keypoints, which leave the oriented list the description reads.  Like
tools/orient_bench.py, the launches rotate over enough independent contexts to exceed 2 GiB of
pyramid, so the windows come from HBM, not from a cache the previous launch filled.  Each
describe_keypoints (counter memset + one kernel) is timed with events on the launch stream, and
detect_extrema, refine_keypoints and orient_keypoints the same way in the same session as yardsticks;
prints one JSON line with the four medians and ranges, the inputs and the records produced.
--capacity raises the keypoint capacity (0: enough for every keypoint found); the orientation and the
description keep twice as many records."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import __graft_entry__ as entry  # noqa: E402

ROTATE_BYTES = 2 << 30


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--S", type=int, default=2)
    ap.add_argument("--octaves", type=int, default=5)
    ap.add_argument("--contrast", type=float, default=50.0)
    ap.add_argument("--edge-ratio", type=float, default=0.0)
    ap.add_argument("--refine-contrast", type=float, default=0.0)
    ap.add_argument("--refine-edge-ratio", type=float, default=10.0)
    ap.add_argument("--capacity", type=int, default=0)
    ap.add_argument("--runs", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
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
    first.detect_extrema(a.contrast, a.edge_ratio, stream=stream)
    stream.synchronize()
    capacity = a.capacity or max(65536, first.keypoint_count(0))
    for c in ctxs:
        c.set_keypoint_capacity(capacity)

    def timed(call):
        ms = []
        for i in range(a.warmup + a.runs):
            c = ctxs[i % rotate]
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record(stream)
            call(c)
            t1.record(stream)
            t1.synchronize()
            if i >= a.warmup:
                ms.append(t0.elapsed_time(t1))
        return ms

    detect = timed(lambda c: c.detect_extrema(a.contrast, a.edge_ratio, stream=stream))
    refine = timed(lambda c: c.refine_keypoints(a.refine_contrast, a.refine_edge_ratio, stream=stream))
    for c in ctxs:  # the orientation and descriptor objects and their buffers exist before anything is timed
        c.orient_keypoints(stream)
        c.describe_keypoints(stream)
    stream.synchronize()
    orient = timed(lambda c: c.orient_keypoints(stream))
    describe = timed(lambda c: c.describe_keypoints(stream))
    found = [c.keypoint_count(0) for c in ctxs]
    kept = [c.refined_count(0) for c in ctxs]
    oriented = [c.oriented_count(0) for c in ctxs]
    described = [c.described_count(0) for c in ctxs]
    assert len(set(found)) == 1 and len(set(kept)) == 1 and len(set(oriented)) == 1 and len(set(described)) == 1, \
        (found, kept, oriented, described)

    def stats(name, ms):
        return {name + "_ms": round(statistics.median(ms), 5), name + "_ms_min": round(min(ms), 5),
                name + "_ms_max": round(max(ms), 5)}

    med = statistics.median(describe)
    print(json.dumps({
        "op": "describe_keypoints", "H": a.n, "W": a.n, "S": a.S, "octaves": first.O, "contrast": a.contrast,
        "edge_ratio": a.edge_ratio, "refine_contrast": a.refine_contrast, "refine_edge_ratio": a.refine_edge_ratio,
        "capacity": capacity, "describe_capacity": 2 * capacity, "rotate": rotate, "pyramid_bytes": first.pyramid_bytes(),
        "runs": a.runs, "found": found[0], "refined": kept[0], "describe_inputs": oriented[0], "described": described[0],
        "ns_per_record": round(1e6 * med / max(1, described[0]), 2),
        **stats("describe", describe), **stats("orient", orient), **stats("refine", refine), **stats("detect", detect),
    }), flush=True)
    for c in ctxs:
        c.close()


if __name__ == "__main__":
    main()
