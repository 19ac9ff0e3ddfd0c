"""Time of gdp_warp_image (homography warp of one input image into the other's frame: the matrix of
the direction, a gather-bilinear sweep over every pixel of the destination frame, the coverage count
and the sum of absolute differences) against what a caller would do today with the images already on
the device.

    python tools/warp_bench.py [--n 4096] [--formats i32,u8] [--runs 20] [--warmup 3]

Workload: an n x n query and an n x n train context filled by the device generator, three models
through gdp_warp_set_model / the fit's record — the identity, a 30-degree rotation about the centre
with small perspective terms, and "none" (the fit's record before any fit) — in direction
train_to_query.  Each call (the one-thread matrix kernel + the sweep) is timed with events on the
launch stream.  The same call on a 1 x 1 frame is the fixed cost.

Baseline, same session, same stream, same timing: torch float32 — the sampling grid built from the
same nine floats with tensor operations, torch.nn.functional.grid_sample (bilinear,
align_corners=True, zero padding), rounding, and the absolute-difference sum against the frame.  Its
rounding differs from the rule's; the largest grey-level difference on pixels both cover is reported
for information only.

Also reported, not gated: the algorithmic bytes (source once, destination frame once, output once)
per second beside --copy-tbs (default 6.29, the copy rate README.md quotes).

Prints one JSON line per format and model."""
import argparse
import ctypes
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import __graft_entry__ as entry  # noqa: E402


def rotation(n, degrees=30.0):
    """Query (x, y) -> train: a rotation about the centre with small perspective terms."""
    import numpy as np

    c, s, m = math.cos(math.radians(degrees)), math.sin(math.radians(degrees)), (n - 1) / 2.0
    h = np.array([[c, -s, m - c * m + s * m], [s, c, m - s * m - c * m], [0.0, 0.0, 1.0]])
    p = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [2e-2 / n, -1e-2 / n, 1.0]])
    return (p @ h).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--formats", default="i32,u8")
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--copy-tbs", type=float, default=6.29)
    a = ap.parse_args()
    if a.runs < 20:
        ap.error("--runs must be at least 20")

    import numpy as np
    import torch
    import torch.nn.functional as nnf

    pkg = entry.load_package()
    stream = torch.cuda.Stream()
    n = a.n

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

    # the fixed cost: the same call on a 1 x 1 frame
    with pkg.PyramidContext(1, 1, S=2) as q1, pkg.PyramidContext(1, 1, S=2) as t1:
        for c in (q1, t1):
            c.set_keypoint_capacity(64)
        q1.match_descriptors(t1, ratio=0.0, stream=stream)
        q1.set_warp_model(np.eye(3, dtype=np.float32))
        q1.warp_image(stream=stream)
        stream.synchronize()
        fixed = timed(lambda: q1.warp_image(stream=stream), a.runs)

    for fmt in a.formats.split(","):
        esz = 1 if fmt == "u8" else 4
        with pkg.PyramidContext(n, n, S=2, octaves=1, input_format=fmt) as q, pkg.PyramidContext(n, n, S=2, octaves=1, input_format=fmt) as t:
            for c in (q, t):
                c.set_keypoint_capacity(64)
            q.fill_synthetic(0x5EED, 0, stream=stream)
            t.fill_synthetic(0x5EED, 1, stream=stream)
            q.match_descriptors(t, ratio=0.0, stream=stream)
            q.warp_image(stream=stream)  # the warp object and its buffer exist before anything is timed
            stream.synchronize()
            dt = torch.uint8 if fmt == "u8" else torch.int32
            # the two images as torch sees them: copies of the contexts' inputs (dense rows: the pitch is n here)
            (qptr, qpitch), (tptr, tpitch) = q.device_input(0), t.device_input(0)
            assert qpitch == n and tpitch == n, (qpitch, tpitch)
            host_q, host_t = (np.zeros((n, n), np.uint8 if fmt == "u8" else np.int32) for _ in range(2))
            rt = ctypes.CDLL("libamdhip64.so")
            rt.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
            for host, ptr in ((host_q, qptr), (host_t, tptr)):
                assert rt.hipMemcpy(host.ctypes.data, ptr, host.nbytes, 2) == 0  # hipMemcpyDeviceToHost (synchronous)
            with torch.cuda.stream(stream):
                tq, tt = torch.from_numpy(host_q).cuda(), torch.from_numpy(host_t).cuda()
                src = tt.to(torch.float32)[None, None]  # the baseline's source stays float32: its conversion is not timed
                ys, xs = torch.meshgrid(torch.arange(n, device="cuda", dtype=torch.float32),
                                        torch.arange(n, device="cuda", dtype=torch.float32), indexing="ij")
            stream.synchronize()

            for name, h in (("identity", np.eye(3, dtype=np.float32)), ("rotation30", rotation(n)), ("none", None)):
                q.set_warp_model(h)
                ours = timed(lambda: q.warp_image(fill=0, stream=stream), a.runs)
                rec = q.warp_record()
                line = {"op": "warp_image", "H": n, "W": n, "format": fmt, "model": name, "runs": a.runs,
                        "tile": list(q.warp_layout()), "covered": int(rec["covered"]), "pixels": int(rec["pixels"]), "sad": int(rec["sad"]),
                        **stats("warp", ours), **stats("warp_1x1_frame", fixed)}
                med = statistics.median(ours)
                bytes_moved = 3 * n * n * esz if h is not None else n * n * esz  # "none": the fill stores only
                line["algorithmic_bytes"] = bytes_moved
                line["algorithmic_tbs"] = round(bytes_moved / (med * 1e-3) / 1e12, 3)
                line["fraction_of_copy_rate"] = round(line["algorithmic_tbs"] / a.copy_tbs, 3)
                if h is not None:
                    m = [float(v) for v in h.reshape(9)]
                    result = {}

                    def baseline():
                        with torch.cuda.stream(stream):
                            u = (m[0] * xs + m[1] * ys) + m[2]
                            v = (m[3] * xs + m[4] * ys) + m[5]
                            w = (m[6] * xs + m[7] * ys) + m[8]
                            sx, sy = u / w, v / w
                            ok = (w > 0) & (sx >= 0) & (sy >= 0) & (sx <= n - 1) & (sy <= n - 1)
                            grid = torch.stack((sx * (2.0 / (n - 1)) - 1.0, sy * (2.0 / (n - 1)) - 1.0), dim=-1)[None]
                            out = torch.round(nnf.grid_sample(src, grid, mode="bilinear", padding_mode="zeros", align_corners=True))[0, 0]
                            out = torch.where(ok, out, torch.zeros_like(out)).to(dt)
                            sad = torch.where(ok, (out.to(torch.int64) - tq.to(torch.int64)).abs(), torch.zeros_like(out, dtype=torch.int64)).sum()
                            result["out"], result["sad"], result["covered"] = out, sad, ok.sum()

                    ref = timed(baseline, a.runs)
                    stream.synchronize()
                    got = q.warped()
                    theirs = result["out"].cpu().numpy()
                    both = (got != 0) & (theirs != 0)
                    line.update(stats("torch_f32", ref))
                    line["torch_covered"] = int(result["covered"])
                    line["max_grey_level_difference"] = int(np.abs(got.astype(np.int64) - theirs.astype(np.int64))[both].max()) if both.any() else 0
                    line["speedup"] = round(statistics.median(ref) / med, 2)
                    line["ranges_overlap"] = not max(ours) < min(ref)
                    line["faster_than_torch"] = max(ours) < min(ref)
                    del result
                    torch.cuda.empty_cache()
                print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
