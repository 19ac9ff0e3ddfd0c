"""ms per steady-state build over shapes and knob values: the table the defaults of GDP_TUNE_KEEP_KERNEL
and GDP_TUNE_KEEP_SIGNS_KERNEL are read off (profiles/keep_kernel_shapes_r08.json, keep_signs_shapes_r11.json).

    python tools/keep_shapes_bench.py --out shapes.json [--tree DIR] [--modes kk0,kk1,kk2,ks0,kz0] [--shapes HxWxB,...]

Per shape (5 octaves, S = 2, bench.py's synthetic non-negative int32 image): enough contexts in rotation to exceed 2 GiB
as in bench.py, and per round and mode three untimed builds of every context, then `iters` rotated builds between two
events on the launch stream; `--rounds` alternated rounds, median and range per mode.  Modes: kk0 / kk1 / kk2
GDP_TUNE_KEEP_KERNEL 0 / 1 / 2 (an explicit value also sets the shape of the launches that skip by the sign map); ks0
GDP_TUNE_KEEP_SIGNS = 0 on the default kernel; kz0 GDP_TUNE_KEEP_ZEROS = 0 (the full build); def the library's defaults;
sup0 GDP_TUNE_KEEP_SUPPORT = 0 on the default kernel, kk1s0 / kk2s0 on kernel 1 / 2 (every other mode leaves that knob at its default); kk1ks0 / kk2ks0 kernel 1 / 2 with
GDP_TUNE_KEEP_SIGNS = 0: launches that make every level-S+2 store.
--tree: another checkout (built) to import the package from, e.g. the parent commit's, for the same table of it."""
import argparse, json, os, statistics, sys

ap = argparse.ArgumentParser()
ap.add_argument("--tree", default=".")
ap.add_argument("--modes", default="kk0,kk1,kk2")
ap.add_argument("--shapes", default="2048x2048x1,1080x1920x8,4096x4096x1,8192x4096x1,4096x4096x4,1080x1920x64,16384x16384x1,4096x4096x64")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--out", required=True)
a = ap.parse_args()
sys.path.insert(0, os.path.abspath(a.tree))
import torch  # noqa
import __graft_entry__ as entry  # noqa

pkg = entry.load_package()
MODES = {"kk0": dict(keep_kernel=0), "kk1": dict(keep_kernel=1), "kk2": dict(keep_kernel=2), "def": {},
         "ks0": dict(keep_signs=0), "kz0": dict(keep_zeros=0), "sup0": dict(keep_support=0),
         "kk1s0": dict(keep_kernel=1, keep_support=0), "kk2s0": dict(keep_kernel=2, keep_support=0),
         "kk1ks0": dict(keep_kernel=1, keep_signs=0), "kk2ks0": dict(keep_kernel=2, keep_signs=0)}
res = {}
stream = torch.cuda.Stream()
for shape in a.shapes.split(","):
    H, W, B = map(int, shape.split("x"))
    first = pkg.PyramidContext(H, W, S=2, octaves=5, batch=B)
    set_bytes = first.pyramid_bytes() + 4 * H * W * B
    rotate = max(1, -(-(2 << 30) // set_bytes))
    ctxs = [first] + [pkg.PyramidContext(H, W, S=2, octaves=5, batch=B) for _ in range(rotate - 1)]
    base = first.tuning()
    for c in ctxs:
        c.fill_synthetic(0x5EED, 0)
        c.sync()
    px = H * W * B
    iters = max(rotate, 200 if px <= (1 << 26) else 40 if px <= (1 << 28) else 12)
    times = {m: [] for m in a.modes.split(",")}
    for _ in range(a.rounds):
        for m in times:
            knobs = dict(keep_kernel=base["keep_kernel"], keep_zeros=1)
            if "keep_signs" in base:
                knobs["keep_signs"] = 1
            if "keep_support" in base:
                knobs["keep_support"] = base["keep_support"]
            knobs.update(MODES[m])
            for c in ctxs:
                c.set_tuning(**knobs)
                c.build(stream); c.build(stream); c.build(stream)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for i in range(iters):
                ctxs[i % rotate].build(stream)
            e1.record(stream)
            e1.synchronize()
            times[m].append(e0.elapsed_time(e1) / iters)
    res[shape] = {"rotate": rotate, "iters": iters, "default_keep_kernel": base["keep_kernel"], "variant": base["variant"],
                  "median_ms": {m: round(statistics.median(t), 5) for m, t in times.items()},
                  "range_ms": {m: [round(min(t), 5), round(max(t), 5)] for m, t in times.items()}}
    print(shape, json.dumps(res[shape]), flush=True)
    for c in ctxs:
        c.close()
    del ctxs, first
    torch.cuda.empty_cache()
with open(a.out, "w") as f:
    json.dump(res, f, indent=1)
