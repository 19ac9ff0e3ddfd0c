"""SIFT descriptors at the C-ABI boundary, on a machine without a GPU: the nine entry points are
declared, exported and bound, reject null handles without touching outputs or the device, the
described record is 176 bytes in C, C++ and numpy alike and starts with a gdp_keypoint_oriented,
gdp_describe_tables (pure host code) returns the rule's radius, weights and rotation table, the
drop-in classes' DescribeKeypoints compiles, and no export of the set takes a mutable context.  No
compute call is made here."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from describe_oracle import ORIENTED_DT, formula_rotation, formula_weights, radius

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "sift-parallel-optimization_amd")
INCLUDE = os.path.join(REPO, "include")

FUNCTIONS = ("gdp_describe_create", "gdp_describe_destroy", "gdp_describe_last_error", "gdp_describe_set_input",
             "gdp_describe_keypoints", "gdp_described_count", "gdp_download_described", "gdp_device_described",
             "gdp_describe_tables")
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
    assert len(FUNCTIONS) == 9
    for name in FUNCTIONS:
        assert name in declared, name
        assert name in exported, name
        assert name in SIGNATURES, name
        assert not name.startswith("gdp_orient")
    assert pkg.lib().gdp_abi_version() == 1
    header = _header()
    assert "#define GDP_ABI_VERSION 1\n" in header
    assert "Out of scope: descriptors." in header and "gdp_describe_keypoints, further below" in header
    for word in ("0x3fa2f890", "0xbed8d61d", "0x3e7c5661", "0xbe17cbe9", "0x3d89486e", "0xbc74784e", "288.0f", "2121"):
        assert word in header, word  # the rule's constants are written into the header


def test_no_export_of_the_set_takes_a_mutable_context():
    """The design constraint: an export whose first parameter is a mutable gdp_ctx* must invalidate
    the clean pyramid (tests/test_keep_zeros_abi.py), so the descriptors' state lives in gdp_describe
    and the context (and the orientation object) is only ever passed const."""
    header = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    protos = {m.group(1): m.group(2) for m in re.finditer(r"\b(gdp_describe\w*|gdp_described_count|gdp_download_described|"
                                                           r"gdp_device_described)\s*\(([^;]*)\)\s*;", header)}
    assert set(FUNCTIONS) <= set(protos)
    for name in FUNCTIONS:
        assert not re.search(r"(?<!const )gdp_ctx\s*\*", protos[name]), (name, protos[name])
        assert not re.search(r"(?<!const )gdp_orient\s*\*", protos[name]), (name, protos[name])
    assert "const gdp_ctx* ctx" in protos["gdp_describe_create"] and "const gdp_orient* src" in protos["gdp_describe_create"]
    with open(os.path.join(PKG, "csrc", "gdp.hip")) as f:
        src = f.read()
    for name in FUNCTIONS:
        m = re.search(r"^[\w \*]+\b%s\(([^)]*)\)" % name, src, re.M)
        assert m, name
        assert not re.search(r"(?<!const )gdp_ctx\s*\*", m.group(1)), (name, m.group(1))
        assert not re.search(r"(?<!const )gdp_orient\s*\*", m.group(1)), (name, m.group(1))


def test_null_handles_are_argument_errors(pkg):
    L = pkg.lib()
    n, m = ctypes.c_size_t(7), ctypes.c_size_t(9)
    recs, count, handle = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
    rec = np.zeros(1, pkg.ORIENTED_DTYPE)
    out = np.zeros(1, pkg.DESCRIBED_DTYPE)
    assert L.gdp_describe_create(ctypes.byref(handle), None, None, 0) == 1 and handle.value is None
    assert L.gdp_describe_create(None, None, None, 16) == 1
    L.gdp_describe_destroy(None)  # a no-op
    assert L.gdp_describe_set_input(None, 0, ctypes.c_void_p(rec.ctypes.data), 1) == 1
    assert L.gdp_describe_keypoints(None, None) == 1
    assert L.gdp_described_count(None, 0, ctypes.byref(n)) == 1
    assert L.gdp_download_described(None, 0, ctypes.c_void_p(out.ctypes.data), 1, ctypes.byref(n), ctypes.byref(m)) == 1
    assert L.gdp_device_described(None, 0, ctypes.byref(recs), ctypes.byref(count)) == 1
    assert n.value == 7 and m.value == 9 and recs.value is None and count.value is None  # outputs untouched
    assert not out.tobytes().strip(b"\0")
    assert isinstance(L.gdp_describe_last_error(None), bytes)
    w = np.full(243, 7.0, np.float32)
    r = ctypes.c_int(-3)
    ptr = ctypes.c_void_p(w.ctypes.data)
    assert L.gdp_describe_tables(2, 1, ptr, None, None, None) == 1  # the radius is required
    for S, s in ((2, 0), (2, 3), (0, 1), (-1, 1)):
        assert L.gdp_describe_tables(S, s, ptr, ctypes.byref(r), None, None) == 1, (S, s)
    assert r.value == -3 and (w == 7.0).all()
    assert L.gdp_describe_tables(2, 1, None, ctypes.byref(r), None, None) == 0 and r.value == 11  # every other output may be NULL


def test_tables_follow_the_rule(pkg):
    C, Sn = formula_rotation()
    for S in (1, 2, 3, 5, 9):
        for s in range(1, S + 1):
            w, R, cosv, sinv = pkg.describe_tables(S, s)
            assert R == radius(s) == (2121 + 50 * (s + 1)) // (100 * (s + 1)) and w.dtype == np.float32 and w.size == 2 * R * R + 1
            want = formula_weights(s)  # the float64 formula rounded to float32; expf may differ in the last bit
            ulp = np.spacing(want)
            assert np.all(np.abs(w.astype(np.float64) - want.astype(np.float64)) <= ulp), (S, s)
            assert w[0] == 1.0 and np.all(np.diff(w) < 0)
            assert np.array_equal(cosv, C) and np.array_equal(sinv, Sn)  # the same table for every scale
    assert [pkg.describe_tables(9, s)[1] for s in range(1, 10)] == [11, 7, 5, 4, 4, 3, 3, 2, 2]
    assert [float(C[a]) for a in (0, 360, 720, 1080)] == [1.0, 0.0, -1.0, 0.0]
    # the buffer of 243 is never exceeded, and nothing past 2R^2 is written
    buf = np.full(256, 7.0, np.float32)
    r = ctypes.c_int()
    assert pkg.lib().gdp_describe_tables(2, 1, ctypes.c_void_p(buf.ctypes.data), ctypes.byref(r), None, None) == 0
    assert r.value == 11 and (buf[243:] == 7.0).all() and (buf[:243] != 7.0).all()
    buf[:] = 7.0
    assert pkg.lib().gdp_describe_tables(2, 2, ctypes.c_void_p(buf.ctypes.data), ctypes.byref(r), None, None) == 0
    assert r.value == 7 and (buf[99:] == 7.0).all() and (buf[:99] != 7.0).all()


def test_described_dtype_matches_the_struct(pkg):
    dt = pkg.DESCRIBED_DTYPE
    assert dt.itemsize == 176
    od = pkg.ORIENTED_DTYPE  # the first 48 bytes are a gdp_keypoint_oriented
    assert dt.names == od.names + ("desc",)
    assert all(dt.fields[n] == od.fields[n] for n in od.names)
    assert dt.fields["desc"][1] == 48 and dt.fields["desc"][0] == np.dtype((np.uint8, (128,)))
    assert all(ORIENTED_DT.fields[n] == od.fields[n] for n in od.names) and ORIENTED_DT.itemsize == od.itemsize == 48


def test_python_surface(pkg):
    for name in ("describe_keypoints", "described_keypoints", "set_describe_input", "set_describe_capacity", "described_count",
                 "device_described"):
        assert callable(getattr(pkg.PyramidContext, name)), name
    for cls in (pkg.GaussPyramid, pkg.GaussPyramid_a512omp, pkg.GaussPyramid_a512xp):
        assert callable(cls.DescribeKeypoints)
    assert callable(pkg.describe_tables)


_LAYOUT = """
#include <stddef.h>
#include "gdp.h"
%s(sizeof(gdp_keypoint_described) == 176, "eleven 16-byte stores per record");
%s(offsetof(gdp_keypoint_described, octave) == offsetof(gdp_keypoint_oriented, octave) &&
   offsetof(gdp_keypoint_described, scale) == offsetof(gdp_keypoint_oriented, scale) &&
   offsetof(gdp_keypoint_described, kind) == offsetof(gdp_keypoint_oriented, kind) &&
   offsetof(gdp_keypoint_described, row) == offsetof(gdp_keypoint_oriented, row) &&
   offsetof(gdp_keypoint_described, col) == offsetof(gdp_keypoint_oriented, col) &&
   offsetof(gdp_keypoint_described, value) == offsetof(gdp_keypoint_oriented, value) &&
   offsetof(gdp_keypoint_described, dscale) == offsetof(gdp_keypoint_oriented, dscale) &&
   offsetof(gdp_keypoint_described, drow) == offsetof(gdp_keypoint_oriented, drow) &&
   offsetof(gdp_keypoint_described, dcol) == offsetof(gdp_keypoint_oriented, dcol) &&
   offsetof(gdp_keypoint_described, interp) == offsetof(gdp_keypoint_oriented, interp) &&
   offsetof(gdp_keypoint_described, angle) == offsetof(gdp_keypoint_oriented, angle) &&
   offsetof(gdp_keypoint_described, peak) == offsetof(gdp_keypoint_oriented, peak) &&
   offsetof(gdp_keypoint_described, bin) == offsetof(gdp_keypoint_oriented, bin) &&
   offsetof(gdp_keypoint_described, peaks) == offsetof(gdp_keypoint_oriented, peaks), "starts with a gdp_keypoint_oriented");
%s(offsetof(gdp_keypoint_described, desc) == sizeof(gdp_keypoint_oriented) && sizeof(gdp_keypoint_oriented) == 48 &&
   sizeof(((gdp_keypoint_described*)0)->desc) == 128, "128 descriptor bytes after the oriented record");
int use(const gdp_ctx* c, const gdp_orient* src, gdp_keypoint_described* k, const gdp_keypoint_oriented* in, size_t n) {
    gdp_describe* w = 0;
    size_t stored = 0, found = 0;
    const gdp_keypoint_described* dev = 0;
    const uint32_t* count = 0;
    float weights[243], cosv[1440], sinv[1440];
    int radius = 0;
    int rc = gdp_describe_create(&w, c, src, 0) + gdp_describe_set_input(w, 0, in, n) + gdp_describe_keypoints(w, 0) +
             gdp_described_count(w, 0, &found) + gdp_download_described(w, 0, k, n, &stored, &found) +
             gdp_device_described(w, 0, &dev, &count) + gdp_describe_tables(2, 1, weights, &radius, cosv, sinv);
    rc += gdp_describe_last_error(w) != 0;
    gdp_describe_destroy(w);
    return rc;
}
"""


@pytest.mark.parametrize("compiler,std,suffix,keyword", [("gcc", "-std=c11", ".c", "_Static_assert"),
                                                          ("g++", "-std=c++14", ".cpp", "static_assert")])
def test_record_is_176_bytes_in_c_and_cxx(tmp_path, compiler, std, suffix, keyword):
    src = tmp_path / ("layout" + suffix)
    src.write_text(_LAYOUT % ((keyword,) * 3))
    subprocess.run([compiler, std] + STRICT + [str(src)], check=True)


_DROPIN = """
#include "%s"
std::vector<gdp_keypoint_described> all(%s& g) { return g.DescribeKeypoints(); }
size_t pipeline(%s& g) {
    g.DetectExtrema(); g.RefineKeypoints(0.03f, 10.f); g.OrientKeypoints();
    return g.DescribeKeypoints().size();
}
"""


@pytest.mark.parametrize("header,cls", [("GaussDePyramid-HIP.h", "GaussPyramid_hip"),
                                        ("GaussDePyramid-HIP-AVX512.h", "GaussPyramid_a512omp_hip"),
                                        ("GaussDePyramid-HIP-AVX512.h", "GaussPyramid_a512xp_hip")])
def test_dropin_describe_keypoints_compiles(tmp_path, header, cls):
    src = tmp_path / "describe.cpp"
    src.write_text(_DROPIN % (header, cls, cls))
    subprocess.run(["g++", "-std=c++14"] + STRICT + [str(src)], check=True)


def test_example_and_tool_are_wired():
    with open(os.path.join(REPO, "examples", "Makefile")) as f:
        mk = f.read()
    assert mk.count("describe_hip") >= 4  # in `all`, its rule (target + source) and `clean`
    assert os.path.exists(os.path.join(REPO, "examples", "describe_hip.cpp"))
    assert os.path.exists(os.path.join(REPO, "tools", "describe_bench.py"))
    with open(os.path.join(PKG, "csrc", "Makefile")) as f:
        mk = f.read()
    assert "DESCRIBE := gdp_describe.inc" in mk and "$(OUT)/libgdp.so asm exp: $(DESCRIBE)" in mk
    assert os.path.exists(os.path.join(PKG, "csrc", "gdp_describe.inc"))
    with open(os.path.join(REPO, ".gitignore")) as f:
        assert "examples/describe_hip\n" in f.read()
