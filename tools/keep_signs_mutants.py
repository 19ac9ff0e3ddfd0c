"""Mutated scratch builds of libgdp.so for the sign-map tests (GDP_TUNE_KEEP_SIGNS, csrc/gdp_keep.inc).

    python3 tools/keep_signs_mutants.py --out DIR            # CPU: write and build DIR/<mutant>/libgdp.so
    python3 tools/keep_signs_mutants.py --out DIR --run      # GPU: the new tests against every built mutant

Each mutant is a copy of csrc/ with one edit of the rule in keep_tile_fast; every one must FAIL both
tests/test_gpu_keep_signs.py (the fixed cases) and tests/test_gpu_keep_signs_fuzz.py (the sweep), run
with GDP_LIBRARY pointing at it (profiles/keep_signs_mutants_r11.log).  The edits change which
stores run and which of the tile's own 16 flag bytes is written; no access leaves its bounds.  The
committed tree is left alone."""
import argparse
import os
import shutil
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "sift-parallel-optimization_amd", "csrc")
TESTS = ("tests/test_gpu_keep_signs.py", "tests/test_gpu_keep_signs_fuzz.py")

BALLOT = "__ballot((x[j].x | x[j].y | x[j].z | x[j].w) < 0) != 0 ? 1u : 0u"
# name -> [(old, new, occurrences)]
MUTANTS = {
    "m1_flag_never_written_in_use": [("if (was != neg && lane == 0", "if (false && was != neg && lane == 0", 1)],
    # both the establishing and the using launch
    "m2_flag_index_off_by_one": [("flags[rt0 + j] = (unsigned char)neg;", "flags[(rt0 + j + 1) & 15] = (unsigned char)neg;", 2)],
    "m3_old_ignored": [("run |= ((was | neg) ? 1u : 0u) << j;", "run |= (neg ? 1u : 0u) << j;", 1)],
    "m4_new_from_lane0": [(BALLOT, "__builtin_amdgcn_readfirstlane(x[j].x | x[j].y | x[j].z | x[j].w) < 0 ? 1u : 0u", 1)],
    # a partly storing wave's octave 1-4 stores follow the neighbouring row's decision (the helper's lines only:
    # eight spaces of indent; the map-free instantiation's loop is left alone)
    "m5_octaves_keyed_to_wrong_row": [
        ("auto store_row = [&](int j) {", "auto store_row = [&](int j, bool d0 = true, bool d1 = true) {", 1),
        ("\n        if ((fast & 1u) && col_ok", "\n        if (d0 && (fast & 1u) && col_ok", 1),
        ("\n        if ((fast & 2u) &&", "\n        if (d1 && (fast & 2u) &&", 1), ("\n        if ((fast & 4u) &&", "\n        if (d1 && (fast & 4u) &&", 1),
        ("\n        if ((fast & 8u) &&", "\n        if (d1 && (fast & 8u) &&", 1), ("\n        if ((fast & 16u) &&", "\n        if (d1 && (fast & 16u) &&", 1),
        ("            if (run >> j & 1u) store_row(j);", "            store_row(j, run >> j & 1u, run >> (j ^ 1) & 1u);", 1),
    ],
}

def build(out):
    with open(os.path.join(CSRC, "gdp_keep.inc")) as f:
        base = f.read()
    for name, edits in MUTANTS.items():
        d = os.path.join(out, name)
        shutil.rmtree(d, ignore_errors=True)
        shutil.copytree(CSRC, os.path.join(d, "csrc"))
        src = base
        for old, new, n in edits:
            assert src.count(old) == n, (name, old, src.count(old))  # the kernel changed: revisit the mutant
            src = src.replace(old, new)
        with open(os.path.join(d, "csrc", "gdp_keep.inc"), "w") as f:
            f.write(src)
    jobs = [subprocess.Popen(["make", "-s", "-C", os.path.join(out, n, "csrc"), "ROOT=" + REPO, "OUT=" + os.path.join(out, n),
                              os.path.join(out, n, "libgdp.so")]) for n in MUTANTS]
    if any(j.wait() for j in jobs):
        sys.exit("a mutant did not build")
    print("built", *(os.path.join(out, n, "libgdp.so") for n in MUTANTS), sep="\n", flush=True)


def run(out):
    caught = True
    for name in MUTANTS:
        for test in TESTS:
            env = dict(os.environ, GDP_LIBRARY=os.path.join(os.path.abspath(out), name, "libgdp.so"))
            r = subprocess.run([sys.executable, "-m", "pytest", "-m", "gpu", "-q", "-x", test], cwd=REPO, env=env,
                               capture_output=True, text=True, timeout=300)
            tail = [ln[:300] for ln in r.stdout.splitlines() if ln.startswith(("FAILED", "E   ")) or " passed" in ln or " failed" in ln]
            print(f"== mutant {name}: {test}: exit status {r.returncode}", *tail[:4], sep="\n", flush=True)
            if r.returncode not in (0, 1):
                sys.exit(f"{name}: {test} ended with status {r.returncode}: stopping")
            caught &= r.returncode == 1
    sys.exit(0 if caught else "a mutant passed")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--run", action="store_true")
    a = ap.parse_args()
    run(a.out) if a.run else build(a.out)
