"""CPU-only checks of GDP_TUNE_KEEP_SUPPORT / GDP_TUNE_KEEP_SUPPORT_UNITS (k_keep's support units,
csrc/gdp_keep.inc): the header documents keys 27 and 28 and the bindings carry them; the units knob
refuses a set; the switch is a kernel argument of the launch — no geometry upload, no drain, and
neither the clean flag nor the sign map is touched; the kernel classifies by the host's tile
rectangles alone."""
import inspect
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "sift-parallel-optimization_amd", "csrc")


def _read(*parts):
    with open(os.path.join(*parts)) as f:
        return f.read()


def test_header_documents_keys_27_and_28_and_the_bindings_carry_them(pkg):
    _lib = __import__(pkg.__name__ + "._lib", fromlist=["_lib"])
    header = _read(REPO, "include", "gdp.h")
    m = re.search(r"GDP_TUNE_KEEP_SUPPORT\s*=\s*27\b,\s*/\*(.*?)\*/", header, re.S)
    assert m, "gdp.h: GDP_TUNE_KEEP_SUPPORT = 27 with its comment"
    doc = " ".join(m.group(1).split())
    for word in ("1 (default)", "k_keep", "support", "units of their own", "0 =", "same bits", "GDP_TUNE_ZEROS_CLEAN",
                 "GDP_TUNE_SIGNS_KNOWN", "no drain"):
        assert word in doc, word
    m = re.search(r"GDP_TUNE_KEEP_SUPPORT_UNITS\s*=\s*28\b,\s*/\*(.*?)\*/", header, re.S)
    assert m, "gdp.h: GDP_TUNE_KEEP_SUPPORT_UNITS = 28 with its comment"
    doc = " ".join(m.group(1).split())
    for word in ("read-only", "k_keep", "GDP_TUNE_KEEP_SUPPORT = 0", "GDP_TUNE_KEEP_KERNEL"):
        assert word in doc, word
    assert _lib.GDP_TUNE_KEEP_SUPPORT == 27 and _lib.GDP_TUNE_KEEP_SUPPORT_UNITS == 28
    # the next free values: no other key of the enum carries them, and none lies above
    values = [int(v) for v in re.findall(r"^\s*GDP_TUNE_[A-Z_]+\s*=\s*(\d+)", header, re.M)]  # the enum's own lines
    assert values.count(27) == 1 and values.count(28) == 1 and max(values) == 28 and len(set(values)) == len(values)
    assert re.search(r"#define GDP_ABI_VERSION 1\b", header)  # new tuning keys are no ABI break
    tuning = pkg.PyramidContext._TUNING
    assert "keep_support" in tuning and "keep_support_units" in tuning
    assert pkg.PyramidContext._tuning_key("keep_support") == 27 and pkg.PyramidContext._tuning_key("keep_support_units") == 28
    params = inspect.signature(pkg.PyramidContext.set_tuning).parameters
    assert "keep_support" in params and "keep_support_units" not in params  # read-only


def test_the_units_knob_refuses_a_set_and_the_switch_touches_nothing_else():
    src = _read(CSRC, "gdp.hip")
    ro = src[src.index("case GDP_TUNE_KEEP_SUPPORT_UNITS:\n            return"):][:200]
    assert "GDP_ERR_ARG" in ro and "read-only" in ro
    case = src[src.index("case GDP_TUNE_KEEP_SUPPORT:\n            if"):]
    case = case[:case.index("case GDP_TUNE_KEEP_SUPPORT_UNITS:")]
    assert "c->keep_support = value;" in case and "value != 0 && value != 1" in case
    for word in ("upload_geom", "hipDeviceSynchronize", "zeros_clean", "signs_unknown", "signs_known", "pyramid_written"):
        assert word not in case, word
    assert re.search(r"int keep_support = 1;", src)  # the default
    # read back: the knob, and the units of the next k_keep launch (0 with the knob off or no k_keep)
    assert "case GDP_TUNE_KEEP_SUPPORT: *value = c->keep_support; return GDP_OK;" in src
    assert "case GDP_TUNE_KEEP_SUPPORT_UNITS: *value = (int)keep_support_units(c); return GDP_OK;" in src
    units = src[src.index("unsigned keep_support_units(const gdp_ctx* c)"):][:300]
    assert "c->keep_support && c->keep_kernel > 0 && g.W % 4 == 0 && g.vec_in" in units and "g.kp_sup_units : 0u" in units


def test_the_switch_is_a_kernel_argument_and_the_grid_counts_the_units():
    src = _read(CSRC, "gdp.hip")
    body = src[src.index("int launch_build("):src.index("template <int MODE, int SUB>")]
    assert "(long long)keep_support_units(c) + g.kp_tiles_total + g.kp_tail_units" in body
    assert "c->d_taps, support, c->d_signs, mode)" in body
    keep = _read(CSRC, "gdp_keep.inc")
    assert re.search(r"k_keep\(const Geom\* __restrict__ g,[^)]*int support, unsigned char\* sign_map, int signs\)", keep, re.S)
    kern = keep[keep.index("__global__ void"):]
    # the support units come first, the grid-stride loop spans all three kinds of unit
    assert "const unsigned sup_units = support ? g->kp_sup_units : 0u;" in kern
    assert kern.index("if (u < sup_units)") < kern.index("if (u >= tiles_end)") < kern.index("keep_tile_fast<")
    assert "u += gridDim.x" in kern
    # one group per thread on either block shape
    unit = keep[keep.index("void keep_support_unit("):keep.index("// The register stores of one tile")]
    assert "if (threadIdx.x >= kTailGroups) return;" in unit and "for (" not in unit
    assert "build_group<0, NT, false>(g, in, out, taps, 1, (int)b, o, og, Rl, C);" in unit
    assert "static_assert(BLK >= kTailGroups" in kern


def test_the_kernel_classifies_by_the_hosts_rectangles_alone():
    keep = _read(CSRC, "gdp_keep.inc")
    kern = keep[keep.index("__global__ void"):]
    assert "sp_r0" not in kern and "sp_c0" not in kern and "sp_r1" not in kern and "sp_c1" not in kern
    for f in ("kp_sl_tr0", "kp_sl_tr1", "kp_sl_tc0", "kp_sl_tc1"):
        assert f in kern, f
    geom = _read(CSRC, "gdp_geom.inc")
    for f in ("kp_sl_tr0[kFused]", "kp_sg_r0[kFused]", "kp_sg_rows[kFused]", "kp_sg_c0[kFused]", "kp_sg_gpr[kFused]",
              "kp_sup_begin[kFused + 1]", "kp_sup_units"):
        assert f in geom, f
    src = _read(CSRC, "gdp.hip")
    host = src[src.index("void keep_support_geom(Geom& g)"):src.index("void set_window_support(")]
    # the predicate k_keep applied per tile, term for term
    assert "r_lo < og.sp_r1 && r_hi > og.sp_r0" in host and "c_lo < og.sp_c1 && c_hi > og.sp_c0" in host
    sup = src[src.index("void set_window_support("):src.index("bool valid_level(")]
    assert "keep_support_geom(g);" in sup  # wherever the support is set, before the geometry is uploaded
