"""Time of gdp_match_guided (matching inside a window round every query's projection, a cell list over
the train frame) against what a caller does today with the lists on the device: the dense sweep of
gdp_match_descriptors on the same two lists.

    python tools/guided_bench.py [--n 4096] [--S 2] [--octaves 5] [--sizes 50:0,40:280615]
                                 [--radius 3] [--runs 20] [--warmup 3]

Workload: tools/match_bench.py's — bench.py's config 2 (one 4096^2 image, S = 2, 5 octaves) after
build_gaussian on the synthetic image, then detect_extrema(contrast), refine_keypoints(0, 10),
orient_keypoints and describe_keypoints, once per entry CONTRAST:KEYPOINT_CAPACITY of --sizes.  The
described list is matched against itself under the identity with `radius` and unique on.  Each call
(the fill, prepare, scan, scatter, search, claim, select) is timed with events on the launch stream,
and so is the yardstick, match_descriptors(ratio=0) on the same lists in the same session on the same
stream.

Sanity: in both runs every query's record must be itself at distance 0 — the list's records that
share a descriptor with an earlier one are counted and excused (the rule sends a tie to the lowest
index).

Prints one JSON line per size with the medians and ranges and whether the two ranges overlap."""
import argparse
import ctypes
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
    ap.add_argument("--radius", type=float, default=3.0)
    ap.add_argument("--max-cells", type=int, default=0)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
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

    def itself(recs, n, first_copy):
        """Every query's record is itself at distance 0 (a copy of an earlier descriptor: that earlier one)."""
        return (len(recs) == n and np.array_equal(recs["query"], np.arange(n, dtype=np.uint32)) and not recs["distance"].any() and
                np.array_equal(recs["train"], first_copy))

    for size in a.sizes.split(","):
        contrast, capacity = size.split(":")
        contrast, capacity = float(contrast), int(capacity)
        with pkg.PyramidContext(a.n, a.n, S=a.S, octaves=a.octaves) as ctx:
            if capacity:
                ctx.set_keypoint_capacity(capacity)
            ctx.set_guided_capacity(a.max_cells)
            ctx.fill_synthetic(0x5EED, 0, stream=stream)
            ctx.build_gaussian(stream)
            ctx.detect_extrema(contrast, 0.0, stream=stream)
            ctx.refine_keypoints(0.0, 10.0, stream=stream)
            ctx.orient_keypoints(stream)
            ctx.describe_keypoints(stream)
            stream.synchronize()
            n = ctx.described_count(0)
            ctx.match_descriptors(ratio=0.0, stream=stream)  # the objects and their buffers exist before anything is timed
            ctx.set_guided_model(np.eye(3, dtype=np.float32))
            ctx.guided_match(a.radius, unique=True, stream=stream)
            stream.synchronize()
            layout = ctx.guided_layout()
            guided = timed(lambda: ctx.guided_match(a.radius, unique=True, stream=stream), a.runs)
            dense = timed(lambda: ctx.match_descriptors(ratio=0.0, stream=stream), a.runs)
            stream.synchronize()
            g, d = np.asarray(ctx.guided_matches()), np.asarray(ctx.matches())
            # records in device order: the lowest index that holds the same descriptor AT THE SAME POSITION is what
            # unique and the tie rule leave; the dense sweep knows no position
            hip = ctypes.CDLL("libamdhip64.so")
            hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
            raw = np.zeros(n, pkg.DESCRIBED_DTYPE)
            assert hip.hipMemcpy(raw.ctypes.data, ctx.device_described(0)[0], raw.nbytes, 2) == 0
            seen, first_desc = {}, np.zeros(n, np.uint32)
            for i in range(n):
                first_desc[i] = seen.setdefault(raw["desc"][i].tobytes(), i)
            copies = int(np.count_nonzero(first_desc != np.arange(n)))
            ok_dense = itself(d, n, first_desc)
            ok_guided = copies == 0 and itself(g, n, first_desc)
            if copies:  # unique drops the later copy where it lies in the earlier one's window: compare on the rest
                keep = np.isin(np.arange(n, dtype=np.uint32), g["query"])
                ok_guided = (not g["distance"].any() and np.array_equal(g["train"], first_desc[g["query"]]) and
                             bool(np.all(keep | (first_desc != np.arange(n)))))
        med_g, med_d = statistics.median(guided), statistics.median(dense)
        print(json.dumps({
            "op": "match_guided", "H": a.n, "W": a.n, "S": a.S, "octaves": a.octaves, "contrast": contrast,
            "keypoint_capacity": capacity or 65536, "nq": n, "nt": n, "radius": a.radius, "unique": True, "runs": a.runs,
            "cell_side": layout[0], "cells": [layout[1], layout[2]], "max_cells": layout[3], "lanes_per_query": layout[4],
            "kept": len(g), "kept_dense": len(d), "copies_of_an_earlier_descriptor": copies,
            "every_query_is_itself_guided": bool(ok_guided), "every_query_is_itself_dense": bool(ok_dense),
            **stats("guided", guided), **stats("dense", dense), "dense_over_guided": round(med_d / med_g, 2),
            "ranges_overlap": not (max(guided) < min(dense) or max(dense) < min(guided)), "guided_faster": max(guided) < min(dense),
        }), flush=True)


if __name__ == "__main__":
    main()
