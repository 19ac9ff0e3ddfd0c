"""Guided matching at the C-ABI boundary, on a machine without a GPU: the entry points are declared,
exported and bound, reject null handles without touching outputs or the device, the output record is
the 32-byte gdp_match_record in C and C++, the rule's key sentences are in the header, create fails
loudly without a GPU, the drop-in classes' GuidedMatch compiles, and no export of the set takes a
mutable context, orientation, describe, match or ransac object.  No compute call is made here."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from match_oracle import MATCH_DT

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "sift-parallel-optimization_amd")
INCLUDE = os.path.join(REPO, "include")

# every *guided* prototype of include/gdp.h
FUNCTIONS = ("gdp_guided_create", "gdp_guided_destroy", "gdp_guided_last_error", "gdp_guided_set_model", "gdp_match_guided",
             "gdp_guided_count", "gdp_download_guided", "gdp_device_guided", "gdp_guided_layout")
STRICT = ["-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I" + INCLUDE]


def _header():
    with open(os.path.join(INCLUDE, "gdp.h")) as f:
        return f.read()


def test_functions_declared_exported_and_bound(pkg):
    from sift_parallel_optimization_amd._lib import SIGNATURES

    declared = pkg.header_functions()
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(PKG, "lib", "libgdp.so")], capture_output=True,
                         text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert sorted(FUNCTIONS) == sorted(f for f in declared if "guided" in f)  # the whole set, nothing beside it
    for name in FUNCTIONS:
        assert name in declared, name
        assert name in exported, name
        assert name in SIGNATURES, name
    assert pkg.lib().gdp_abi_version() == 1
    header = _header()
    assert "#define GDP_ABI_VERSION 1\n" in header
    for word in ("u = (h0 * qx + h1 * qy) + h2,  v = (h3 * qx + h4 * qy) + h5,  w = (h6 * qx + h7 * qy) + h8", "!(w > 0)",
                 "IEEE correctly rounded divisions", "x0 = sx - r, x1 = sx + r, y0 = sy - r, y1 = sy + r",
                 "x0 <= tx_j && tx_j <= x1 && y0 <= ty_j && ty_j <= y1", "a NaN anywhere fails", "(dist(i, j), j) lexicographically",
                 "0xffffffff with a single candidate", "(float)0xffffffff is 2^32", "minimises (distance, query) lexicographically",
                 "clamped into the grid in float before the conversion to integer", "a NaN coordinate is in no cell",
                 "clamp(floorf(x * (1 / c)), 0, G - 1)", "any 176", "radius` must be finite and >= 0"):
        assert word in header, word  # the rule is written into the header


def test_no_export_of_the_set_takes_a_mutable_upstream_handle():
    header = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    protos = {m.group(1): m.group(2) for m in re.finditer(r"\b(gdp_\w+)\s*\(([^;]*)\)\s*;", header)}
    assert set(FUNCTIONS) <= set(protos)
    with open(os.path.join(PKG, "csrc", "gdp.hip")) as f:
        src = f.read()
    for name in FUNCTIONS:
        m = re.search(r"^[\w \*]+\b%s\(([^)]*)\)" % name, src, re.M)
        assert m, name
        for params in (protos[name], m.group(1)):
            for handle in ("gdp_ctx", "gdp_orient", "gdp_describe", "gdp_match", "gdp_ransac"):
                assert not re.search(r"(?<!const )%s\s*\*" % handle, params), (name, params)
    assert protos["gdp_guided_create"].count("const gdp_ransac*") == 1
    for name in ("gdp_device_guided", "gdp_guided_layout", "gdp_guided_last_error"):
        assert "const gdp_guided*" in protos[name], name


def test_null_handles_are_argument_errors(pkg):
    L = pkg.lib()
    n = [ctypes.c_size_t(7) for _ in range(2)]
    u = [ctypes.c_uint32(5) for _ in range(4)]
    side = ctypes.c_float(2.5)
    recs, count, handle = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
    out = np.zeros(4, pkg.MATCH_DTYPE)
    h = np.eye(3, dtype=np.float32)
    assert L.gdp_guided_create(ctypes.byref(handle), None, 0) == 1 and handle.value is None  # a NULL fit object
    assert L.gdp_guided_create(None, None, 0) == 1
    L.gdp_guided_destroy(None)  # a no-op
    assert L.gdp_guided_set_model(None, ctypes.c_void_p(h.ctypes.data)) == 1
    assert L.gdp_match_guided(None, 0, 0, 3.0, 0.0, 0xffffffff, 1, None) == 1
    assert L.gdp_guided_count(None, ctypes.byref(n[0])) == 1
    assert L.gdp_download_guided(None, ctypes.c_void_p(out.ctypes.data), 4, ctypes.byref(n[0]), ctypes.byref(n[1])) == 1
    assert L.gdp_device_guided(None, ctypes.byref(recs), ctypes.byref(count)) == 1
    assert L.gdp_guided_layout(None, ctypes.byref(side), *[ctypes.byref(x) for x in u]) == 1
    assert [x.value for x in n] == [7, 7] and [x.value for x in u] == [5] * 4 and side.value == 2.5  # outputs untouched
    assert recs.value is None and count.value is None and not out.tobytes().strip(b"\0")
    assert isinstance(L.gdp_guided_last_error(None), bytes)


def test_create_fails_loudly_without_a_gpu(pkg):
    """Without a device the chain fails where it starts, at the context, with an error and never a
    CPU result: there is no fit object to create a guided object from."""
    if pkg.lib().gdp_device_count() > 0:  # with a device: two empty lists, no record
        with pkg.PyramidContext(40, 56, S=2, octaves=2) as ctx:
            ctx.guided_match(3.0)
            assert ctx.guided_count() == 0 and len(ctx.guided_matches()) == 0
        return
    with pytest.raises(pkg.GdpError):
        with pkg.PyramidContext(40, 56, S=2, octaves=2) as ctx:
            ctx.guided_match(3.0)


def test_the_record_is_the_match_record(pkg):
    dt = pkg.MATCH_DTYPE
    assert dt.itemsize == 32 and MATCH_DT.itemsize == 32 and all(MATCH_DT.fields[n] == dt.fields[n] for n in dt.names)


def test_python_surface(pkg):
    for name in ("guided_match", "guided_matches", "guided_count", "device_guided", "set_guided_model", "guided_layout",
                 "set_guided_capacity"):
        assert callable(getattr(pkg.PyramidContext, name)), name
    for cls in (pkg.GaussPyramid, pkg.GaussPyramid_a512omp, pkg.GaussPyramid_a512xp):
        assert callable(cls.GuidedMatch)
    from sift_parallel_optimization_amd._lib import check

    # a failed create is reported with gdp_guided_last_error(None), or the status string when that is empty
    handle = ctypes.c_void_p()
    with pytest.raises(pkg.GdpError) as err:
        check(pkg.lib().gdp_guided_create(ctypes.byref(handle), None, 0), None, "guided")
    text = pkg.lib().gdp_guided_last_error(None) or pkg.lib().gdp_status_string(1)
    assert err.value.status == 1 and handle.value is None and str(err.value) == "libgdp status 1: " + text.decode()
    with pytest.raises(ValueError):
        pkg.PyramidContext.set_guided_capacity(None, -1)


_LAYOUT = """
#include <stddef.h>
#include "gdp.h"
%s(sizeof(gdp_match_record) == 32, "the existing 32-byte record");
int use(const gdp_ransac* src, const float* h9, gdp_match_record* host, size_t n) {
    gdp_guided* g = 0;
    const gdp_match_record* dev = 0;
    const uint32_t* count = 0;
    size_t stored = 0, found = 0;
    float side = 0;
    uint32_t gx = 0, gy = 0, most = 0, lanes = 0;
    int rc = gdp_guided_create(&g, src, 0) + gdp_guided_set_model(g, h9) + gdp_match_guided(g, 0, 0, 3.0f, 0.0f, 0xffffffffu, 1, 0) +
             gdp_guided_count(g, &found) + gdp_download_guided(g, host, n, &stored, &found) + gdp_device_guided(g, &dev, &count) +
             gdp_guided_layout(g, &side, &gx, &gy, &most, &lanes);
    rc += gdp_guided_last_error(g) != 0;
    gdp_guided_destroy(g);
    return rc;
}
"""


@pytest.mark.parametrize("compiler,std,suffix,keyword", [("gcc", "-std=c11", ".c", "_Static_assert"),
                                                          ("g++", "-std=c++14", ".cpp", "static_assert")])
def test_record_is_32_bytes_in_c_and_cxx(tmp_path, compiler, std, suffix, keyword):
    src = tmp_path / ("layout" + suffix)
    src.write_text(_LAYOUT % keyword)
    subprocess.run([compiler, std] + STRICT + [str(src)], check=True)


_DROPIN = """
#include "%s"
std::vector<gdp_match_record> guided(%s& a, %s& b) {
    const gdp_homography H = a.FitHomography(a.MatchDescriptors(b));
    return a.GuidedMatch(b, H.h, 3.0f, 0.8f, 0xffffffffu, true);
}
size_t defaults(%s& g, const float* h) { return g.GuidedMatch(g, h).size(); }
"""


@pytest.mark.parametrize("header,cls", [("GaussDePyramid-HIP.h", "GaussPyramid_hip"),
                                        ("GaussDePyramid-HIP-AVX512.h", "GaussPyramid_a512omp_hip"),
                                        ("GaussDePyramid-HIP-AVX512.h", "GaussPyramid_a512xp_hip")])
def test_dropin_guided_match_compiles(tmp_path, header, cls):
    src = tmp_path / "guided.cpp"
    src.write_text(_DROPIN % (header, cls, cls, cls))
    subprocess.run(["g++", "-std=c++14"] + STRICT + [str(src)], check=True)


def test_example_and_tool_are_wired():
    with open(os.path.join(REPO, "examples", "Makefile")) as f:
        mk = f.read()
    assert mk.count("guided_hip") >= 4  # in `all`, its rule (target + source) and `clean`
    assert os.path.exists(os.path.join(REPO, "examples", "guided_hip.cpp"))
    assert os.path.exists(os.path.join(REPO, "tools", "guided_bench.py"))
    with open(os.path.join(PKG, "csrc", "Makefile")) as f:
        mk = f.read()
    assert "GUIDED := gdp_guided.inc" in mk and "$(OUT)/libgdp.so asm exp: $(GUIDED)" in mk
    with open(os.path.join(PKG, "csrc", "gdp.hip")) as f:
        assert '#include "gdp_guided.inc"' in f.read()
    with open(os.path.join(REPO, ".gitignore")) as f:
        assert "examples/guided_hip\n" in f.read()
    for doc, word in (("README.md", "gdp_match_guided"), ("DESIGN.md", "5.12"), ("INTEGRATION.md", "GuidedMatch")):
        with open(os.path.join(REPO, doc)) as f:
            assert word in f.read(), (doc, word)
