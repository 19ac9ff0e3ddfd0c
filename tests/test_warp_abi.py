"""The homography warp at the C-ABI boundary, on a machine without a GPU: the entry points are
declared, exported and bound, reject null handles without touching outputs or the device, the warp
record is 64 bytes in C, C++ and numpy alike with `sad` at offset 48, the rule's key sentences are in
the header, the drop-in classes' WarpImage compiles, and no export of the set takes a mutable context,
orientation, describe, match or ransac object.  No compute call is made here."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from warp_oracle import WARP_DT

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "sift-parallel-optimization_amd")
INCLUDE = os.path.join(REPO, "include")

# every gdp_warp_* / *_warp* / *_warped prototype of include/gdp.h
FUNCTIONS = ("gdp_warp_create", "gdp_warp_destroy", "gdp_warp_last_error", "gdp_warp_set_model", "gdp_warp_image",
             "gdp_download_warp_record", "gdp_download_warped", "gdp_device_warped", "gdp_warp_layout")
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
    assert sorted(FUNCTIONS) == sorted(f for f in declared if "warp" in f)  # the whole set, nothing beside it
    for name in FUNCTIONS:
        assert name in declared, name
        assert name in exported, name
        assert name in SIGNATURES, name
    assert pkg.lib().gdp_abi_version() == 1
    header = _header()
    assert "#define GDP_ABI_VERSION 1\n" in header
    assert "any 32 bytes are a valid record" in header  # the earlier steps' sentences stay
    for word in ("GDP_WARP_TRAIN_TO_QUERY = 0, GDP_WARP_QUERY_TO_TRAIN = 1", "hypothesis == 0xffffffff",
                 "det = (h[0] * adj[0][0] + h[1] * adj[1][0]) + h[2] * adj[2][0]", "ldexp(G, -e)", "G is negated when det < 0",
                 "u = (m0 * x + m1 * y) + m2,  v = (m3 * x + m4 * y) + m5,  w = (m6 * x + m7 * y) + m8", "If !(w > 0)",
                 "two IEEE correctly", "sx >= 0 && sy >= 0 && sx <= (float)(Ws - 1) && sy <= (float)(Hs - 1)", "a NaN fails",
                 "x1 = min(x0 + 1, Ws - 1)", "top = p00 + fx * (p01 - p00),  bot = p10 + fx * (p11 - p10)", "val = top + fy * (bot - top)",
                 "q = rintf(val) (ties to even)", "INT32_MAX when q >= 2147483648.0f", "clamped to 0..255",
                 "exact uint64 integer sum", "no address is formed from anything but indices the coverage test has bounded",
                 "GDP_ERR_STATE"):
        assert word in header, word  # the rule is written into the header


def test_no_export_of_the_set_takes_a_mutable_upstream_handle():
    """The design constraint of the earlier stages, one object further: the warp only reads the fit
    object and the two contexts, so the build that follows the whole chain is still the steady-state one."""
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
    assert protos["gdp_warp_create"].count("const gdp_ransac*") == 1
    for name in ("gdp_device_warped", "gdp_warp_layout", "gdp_warp_last_error"):
        assert "const gdp_warp*" in protos[name], name


def test_null_handles_are_argument_errors(pkg):
    L = pkg.lib()
    pitch = ctypes.c_size_t(7)
    i = [ctypes.c_int(5) for _ in range(3)]
    u = [ctypes.c_uint32(5) for _ in range(3)]
    pix, rec_ptr, handle = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
    rec = np.zeros(1, pkg.WARP_DTYPE)
    img = np.zeros(16, np.int32)
    h = np.eye(3, dtype=np.float32)
    assert L.gdp_warp_create(ctypes.byref(handle), None) == 1 and handle.value is None
    assert L.gdp_warp_create(None, None) == 1
    L.gdp_warp_destroy(None)  # a no-op
    assert L.gdp_warp_set_model(None, ctypes.c_void_p(h.ctypes.data)) == 1
    assert L.gdp_warp_image(None, 0, 0, 0, 0, None) == 1
    assert L.gdp_download_warp_record(None, ctypes.c_void_p(rec.ctypes.data)) == 1
    assert L.gdp_download_warped(None, ctypes.c_void_p(img.ctypes.data), 4) == 1
    assert L.gdp_device_warped(None, ctypes.byref(pix), ctypes.byref(pitch), *[ctypes.byref(x) for x in i], ctypes.byref(rec_ptr)) == 1
    assert L.gdp_warp_layout(None, *[ctypes.byref(x) for x in u]) == 1
    assert pitch.value == 7 and pix.value is None and rec_ptr.value is None  # outputs untouched
    assert [x.value for x in i] == [5, 5, 5] and [x.value for x in u] == [5, 5, 5]
    assert not rec.tobytes().strip(b"\0") and not img.any()
    assert isinstance(L.gdp_warp_last_error(None), bytes)


def test_warp_dtype_matches_the_struct(pkg):
    dt = pkg.WARP_DTYPE
    assert dt.itemsize == 64 and dt.names == ("m", "model", "covered", "pixels", "sad", "direction", "reserved")
    assert [dt.fields[n][1] for n in dt.names] == [0, 36, 40, 44, 48, 56, 60]
    assert dt.fields["m"][0] == np.dtype((np.float32, (9,))) and dt.fields["sad"][0] == np.uint64
    assert all(dt.fields[n][0] == np.uint32 for n in ("model", "covered", "pixels", "direction", "reserved"))
    assert all(WARP_DT.fields[n] == dt.fields[n] for n in dt.names) and WARP_DT.itemsize == 64


def test_python_surface(pkg):
    for name in ("warp_image", "warped", "warp_record", "set_warp_model", "device_warped", "warp_layout"):
        assert callable(getattr(pkg.PyramidContext, name)), name
    for cls in (pkg.GaussPyramid, pkg.GaussPyramid_a512omp, pkg.GaussPyramid_a512xp):
        assert callable(cls.WarpImage)
    from sift_parallel_optimization_amd._lib import check

    # a failed create is reported with gdp_warp_last_error(None), or the status string when that is empty
    handle = ctypes.c_void_p()
    with pytest.raises(pkg.GdpError) as err:
        check(pkg.lib().gdp_warp_create(ctypes.byref(handle), None), None, "warp")
    text = pkg.lib().gdp_warp_last_error(None) or pkg.lib().gdp_status_string(1)
    assert err.value.status == 1 and handle.value is None and str(err.value) == "libgdp status 1: " + text.decode()
    from sift_parallel_optimization_amd.gausspyramid import WARP_DIRECTIONS

    assert WARP_DIRECTIONS == {"train_to_query": 0, "query_to_train": 1}
    # the warp handle goes wherever the fit handle goes: tests/test_binding_lifetime.py


_LAYOUT = """
#include <stddef.h>
#include "gdp.h"
%s(sizeof(gdp_warp_record) == 64, "one 64-byte record");
%s(offsetof(gdp_warp_record, m) == 0 && offsetof(gdp_warp_record, model) == 36 && offsetof(gdp_warp_record, covered) == 40 &&
   offsetof(gdp_warp_record, pixels) == 44 && offsetof(gdp_warp_record, sad) == 48 && offsetof(gdp_warp_record, direction) == 56 &&
   offsetof(gdp_warp_record, reserved) == 60, "nine floats, three words, the 8-byte sum at 48, two words");
%s(GDP_WARP_TRAIN_TO_QUERY == 0 && GDP_WARP_QUERY_TO_TRAIN == 1, "the two directions");
int use(const gdp_ransac* src, const float* h9, void* host, gdp_warp_record* rec) {
    gdp_warp* w = 0;
    const void* pixels = 0;
    const gdp_warp_record* dev = 0;
    size_t pitch = 0;
    int height = 0, width = 0, format = 0;
    uint32_t tr = 0, tc = 0, ppl = 0;
    int rc = gdp_warp_create(&w, src) + gdp_warp_set_model(w, h9) + gdp_warp_image(w, GDP_WARP_QUERY_TO_TRAIN, 0, 0, -1, 0) +
             gdp_download_warp_record(w, rec) + gdp_download_warped(w, host, 64) +
             gdp_device_warped(w, &pixels, &pitch, &height, &width, &format, &dev) + gdp_warp_layout(w, &tr, &tc, &ppl);
    rc += gdp_warp_last_error(w) != 0;
    gdp_warp_destroy(w);
    return rc;
}
"""


@pytest.mark.parametrize("compiler,std,suffix,keyword", [("gcc", "-std=c11", ".c", "_Static_assert"),
                                                          ("g++", "-std=c++14", ".cpp", "static_assert")])
def test_record_is_64_bytes_in_c_and_cxx(tmp_path, compiler, std, suffix, keyword):
    src = tmp_path / ("layout" + suffix)
    src.write_text(_LAYOUT % ((keyword,) * 3))
    subprocess.run([compiler, std] + STRICT + [str(src)], check=True)


_DROPIN = """
#include "%s"
std::vector<int32_t> warp(%s& a, %s& b, gdp_warp_record* rec, int* rows, int* cols) {
    const gdp_homography H = a.FitHomography(a.MatchDescriptors(b));
    return a.WarpImage(b, H.h, GDP_WARP_QUERY_TO_TRAIN, -1, rec, rows, cols);
}
size_t defaults(%s& g, const float* h) { return g.WarpImage(g, h).size(); }
"""


@pytest.mark.parametrize("header,cls", [("GaussDePyramid-HIP.h", "GaussPyramid_hip"),
                                        ("GaussDePyramid-HIP-AVX512.h", "GaussPyramid_a512omp_hip"),
                                        ("GaussDePyramid-HIP-AVX512.h", "GaussPyramid_a512xp_hip")])
def test_dropin_warp_image_compiles(tmp_path, header, cls):
    src = tmp_path / "warp.cpp"
    src.write_text(_DROPIN % (header, cls, cls, cls))
    subprocess.run(["g++", "-std=c++14"] + STRICT + [str(src)], check=True)


def test_example_and_tool_are_wired():
    with open(os.path.join(REPO, "examples", "Makefile")) as f:
        mk = f.read()
    assert mk.count("warp_hip") >= 4  # in `all`, its rule (target + source) and `clean`
    assert os.path.exists(os.path.join(REPO, "examples", "warp_hip.cpp"))
    assert os.path.exists(os.path.join(REPO, "tools", "warp_bench.py"))
    with open(os.path.join(PKG, "csrc", "Makefile")) as f:
        mk = f.read()
    assert "WARP := gdp_warp.inc" in mk and "$(OUT)/libgdp.so asm exp: $(WARP)" in mk
    with open(os.path.join(PKG, "csrc", "gdp.hip")) as f:
        assert '#include "gdp_warp.inc"' in f.read()
    with open(os.path.join(REPO, ".gitignore")) as f:
        assert "examples/warp_hip\n" in f.read()
    for doc, word in (("README.md", "gdp_warp_image"), ("DESIGN.md", "5.11"), ("INTEGRATION.md", "WarpImage")):
        with open(os.path.join(REPO, doc)) as f:
            assert word in f.read(), (doc, word)
