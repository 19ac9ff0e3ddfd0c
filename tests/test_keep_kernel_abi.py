"""CPU-only checks of GDP_TUNE_KEEP_KERNEL (the steady-state build's own kernel, csrc/gdp_keep.inc):
the header documents key 23 and the ctypes table and the Python wrapper carry it; libgdp.so still
builds with its Makefile for gfx950 and holds the new kernel; the research builds' preprocessor
branches still compile; launch_build takes the new kernel only for a kept build."""
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "sift-parallel-optimization_amd")
CSRC = os.path.join(PKG, "csrc")


def _hipcc():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.fail("hipcc not found: the builds cannot be checked")
    return hipcc


def test_header_documents_key_23_and_the_bindings_carry_it(pkg):
    _lib = __import__(pkg.__name__ + "._lib", fromlist=["_lib"])
    with open(os.path.join(REPO, "include", "gdp.h")) as f:
        header = f.read()
    m = re.search(r"GDP_TUNE_KEEP_KERNEL\s*=\s*23\b\s*/\*(.*?)\*/", header, re.S)
    assert m, "gdp.h: GDP_TUNE_KEEP_KERNEL = 23 with its comment"
    doc = " ".join(m.group(1).split())
    for word in ("0 =", "k_keep", "multiple of 4", "same bits"):
        assert word in doc, word
    assert _lib.GDP_TUNE_KEEP_KERNEL == 23
    assert re.search(r"GDP_TUNE_KEEP_ZEROS\s*=\s*21\b", header) and re.search(r"GDP_TUNE_ZEROS_CLEAN\s*=\s*22\b", header)
    assert re.search(r"#define GDP_ABI_VERSION 1\b", header)  # a new tuning key is no ABI break
    assert "keep_kernel" in pkg.PyramidContext._TUNING
    assert pkg.PyramidContext._tuning_key("keep_kernel") == 23
    import inspect

    assert "keep_kernel" in inspect.signature(pkg.PyramidContext.set_tuning).parameters


def test_launch_build_takes_the_keep_kernel_only_for_a_kept_build():
    with open(os.path.join(CSRC, "gdp.hip")) as f:
        src = f.read()
    assert '#include "gdp_keep.inc"' in src
    body = src[src.index("int launch_build("):src.index("template <int MODE, int SUB>")]
    # eligibility: a kept build (`keep`), the knob, whole 4-pixel groups, vector loads
    assert re.search(r"if \(keep && c->keep_kernel > 0 && g\.W % 4 == 0 && g\.vec_in\)", body)
    assert body.index("keep = (!subset") < body.index("c->keep_kernel > 0") < body.index("kVariants[")
    # the set path validates against the kernel table and touches neither the geometry nor the flag
    case = src[src.index("case GDP_TUNE_KEEP_KERNEL:\n            if"):]
    case = case[:case.index("case GDP_TUNE_ZEROS_CLEAN:")]
    assert "kNumKeepKernels" in case and "upload_geom" not in case and "zeros_clean" not in case
    with open(os.path.join(CSRC, "Makefile")) as f:
        assert "gdp_keep.inc" in f.read()  # a change to the kernel rebuilds the library


def test_libgdp_builds_with_its_makefile_and_holds_the_kernel(tmp_path):
    """`make -C csrc` for gfx950 into a scratch directory (the committed tree is left alone)."""
    out = tmp_path / "lib"
    subprocess.run(["make", "-C", CSRC, "HIPCC=" + _hipcc(), "ARCH=gfx950", "OUT=" + str(out), str(out / "libgdp.so")],
                   check=True, timeout=900, capture_output=True)
    lib = out / "libgdp.so"
    assert lib.exists()
    syms = subprocess.run(["nm", "-D", "--defined-only", str(lib)], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT gdp_set_tuning$", syms, re.M) and re.search(r"\bT gdp_build$", syms, re.M)
    with open(lib, "rb") as f:
        blob = f.read()
    assert b"k_keep" in blob and b"k_build" in blob  # both kernels' (mangled) names are in the code object


def test_research_build_branches_compile():
    """-DGDP_EXPERIMENTS, -DGDP_TRACE_BLOCKS and the store-policy builds (-DGDP_STORE_POLICY, which
    st_f4<NT> and so k_keep's octave-0 stores honour): one front-end pass over gdp.hip."""
    subprocess.run([_hipcc(), "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-fsyntax-only", "-Wall",
                    "-Wextra", "-Wno-unused-parameter", "-Wno-pass-failed", "-I" + os.path.join(REPO, "include"),
                    "-DGDP_EXPERIMENTS", "-DGDP_TRACE_BLOCKS", "-DGDP_STORE_POLICY=\"sc0 sc1\"",
                    os.path.join(CSRC, "gdp.hip")], check=True, timeout=600)
