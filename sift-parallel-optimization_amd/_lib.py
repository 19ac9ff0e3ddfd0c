"""ctypes binding of libgdp.so — the C ABI declared in include/gdp.h.

The product path is the HIP library; there is no CPU fallback.  If libgdp.so is missing or a
call fails, this module raises GdpError — loudly, never silently computing elsewhere: check() turns a
status into the error, with the last error text of the object the call was made on (LAST_ERROR names
the export per kind of handle: the context and the six stage objects).

HIP runtime sharing: the PyTorch-ROCm wheel ships its own libamdhip64.so (soname
libamdhip64.so.7).  libgdp.so needs `libamdhip64.so.7`; when torch is imported FIRST, the dynamic
loader resolves that soname to torch's already-loaded runtime, so torch streams/events and
libgdp launches share one HIP runtime (and one device context).  Loading libgdp first would map
/opt/rocm's runtime and torch would later map a second one.  We therefore import torch (when it
is installed) before dlopen-ing libgdp; GDP_NO_TORCH=1 skips that for torch-free processes.
"""
import ctypes
import os
import re

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GDP_LIBRARY", os.path.join(PKG_DIR, "lib", "libgdp.so"))
HEADER = os.path.join(os.path.dirname(PKG_DIR), "include", "gdp.h")

GDP_OK, GDP_ERR_ARG, GDP_ERR_HIP, GDP_ERR_STATE, GDP_ERR_NOMEM, GDP_ERR_NODEV, GDP_ERR_INTERNAL = range(7)
GDP_CENTRE_SERIAL, GDP_CENTRE_INTLEN = 0, 1
GDP_INPUT_I32, GDP_INPUT_U8 = 0, 1
GDP_TUNE_NONTEMPORAL, GDP_TUNE_BLOCKS_PER_CU, GDP_TUNE_GRID, GDP_TUNE_VARIANT, GDP_TUNE_TILE_ORDER = 1, 2, 3, 4, 5
GDP_TUNE_INPLACE_SUB, GDP_TUNE_WINDOW_SUB, GDP_TUNE_CONV_KERNEL, GDP_TUNE_CONV_ROWS = 6, 7, 8, 9
GDP_TUNE_CONV_ORDER, GDP_TUNE_BUILD_LDS, GDP_TUNE_STAGE_KB, GDP_TUNE_STAGE_THREADS = 11, 12, 13, 14
GDP_TUNE_CONV_WAVES = 15
GDP_TUNE_ZERO_WINDOW = 16
GDP_TUNE_STORE_PACE = 17
GDP_TUNE_CONV_PACE = 18
GDP_TUNE_INPLACE_PACE = 19
GDP_TUNE_PYRAMID_CHUNK_KB = 20
GDP_TUNE_KEEP_ZEROS = 21
GDP_TUNE_ZEROS_CLEAN = 22
GDP_TUNE_KEEP_KERNEL = 23
GDP_TUNE_KEEP_SIGNS = 24
GDP_TUNE_SIGNS_KNOWN = 25
GDP_TUNE_KEEP_SIGNS_KERNEL = 26
GDP_TUNE_KEEP_SUPPORT = 27
GDP_TUNE_KEEP_SUPPORT_UNITS = 28


class GdpError(RuntimeError):
    """A libgdp call returned a non-zero status (or the library could not be loaded)."""

    def __init__(self, status, message):
        super().__init__(f"libgdp status {status}: {message}")
        self.status = status


_lib = None

_c_int, _c_size, _p, _c_u32, _c_long = ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_long
_pp = ctypes.POINTER(ctypes.c_void_p)

# name -> (restype, argtypes); mirrors include/gdp.h one to one (tests/test_abi.py checks both ways)
SIGNATURES = {
    "gdp_abi_version": (_c_int, []),
    "gdp_octaves_for": (_c_int, [_c_int]),
    "gdp_device_count": (_c_int, []),
    "gdp_create": (_c_int, [_pp, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int]),
    "gdp_create_band": (_c_int, [_pp, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int]),
    "gdp_destroy": (None, [_p]),
    "gdp_get_geometry": (_c_int, [_p] + [ctypes.POINTER(_c_int)] * 5),
    "gdp_level_dims": (_c_int, [_p, _c_int] + [ctypes.POINTER(_c_int)] * 3),
    "gdp_pyramid_bytes": (_c_size, [_p]),
    "gdp_set_input_rows": (_c_int, [_p, _c_int, _p, _p]),
    "gdp_set_input_host": (_c_int, [_p, _c_int, _p, _c_size, _p]),
    "gdp_set_input_device": (_c_int, [_p, _p, _c_size, _c_size]),
    "gdp_set_input_format": (_c_int, [_p, _c_int]),
    "gdp_get_input_format": (_c_int, [_p]),
    "gdp_set_input_host_u8": (_c_int, [_p, _c_int, _p, _c_size, _p]),
    "gdp_set_input_device_u8": (_c_int, [_p, _p, _c_size, _c_size]),
    "gdp_fill_synthetic": (_c_int, [_p, _c_u32, _c_long, _p]),
    "gdp_build": (_c_int, [_p, _p]),
    "gdp_build_gaussian": (_c_int, [_p, _p]),
    "gdp_conv_taps": (_c_int, [_c_int, _c_int, _p, ctypes.POINTER(_c_int)]),
    "gdp_conv_halo_rows": (_c_int, [_p, ctypes.POINTER(_c_int), ctypes.POINTER(_c_int)]),
    "gdp_input_halo": (_c_int, [_p, _c_int, _pp, ctypes.POINTER(_c_size)]),
    "gdp_bind_input_halo": (_c_int, [_p, _p, _p, _c_size, _c_size]),
    "gdp_device_input": (_c_int, [_p, _c_int, _pp, ctypes.POINTER(_c_size)]),
    "gdp_init": (_c_int, [_p, _p]),
    "gdp_gauss_octave": (_c_int, [_p, _c_int, _p]),
    "gdp_gauss_range": (_c_int, [_p, _c_int, _c_int, _p]),
    "gdp_gauss_scales": (_c_int, [_p, _c_int, _c_int, _c_int, _c_int, _p]),
    "gdp_dog_octave": (_c_int, [_p, _c_int, _p]),
    "gdp_dog_range": (_c_int, [_p, _c_int, _c_int, _p]),
    "gdp_generate_dog": (_c_int, [_p, _p]),
    "gdp_build_subset": (_c_int, [_p, _p]),
    "gdp_generate_dog_subset": (_c_int, [_p, _p]),
    "gdp_device_level": (_p, [_p, _c_int, _c_int, _c_int]),
    "gdp_pyramid_written": (_c_int, [_p, _c_int]),
    "gdp_download_level": (_c_int, [_p, _c_int, _c_int, _c_int, _p]),
    "gdp_download_level_rows": (_c_int, [_p, _c_int, _c_int, _c_int, _p]),
    "gdp_download_level_range": (_c_int, [_p, _c_int, _c_int, _c_int, _c_int, _c_int, _p]),
    "gdp_download_pyramid_rows": (_c_int, [_p, _c_int, _p]),
    "gdp_download_pyramid": (_c_int, [_p, _c_int, _p]),
    "gdp_upload_pyramid": (_c_int, [_p, _c_int, _p]),
    "gdp_upload_level": (_c_int, [_p, _c_int, _c_int, _c_int, _p]),
    "gdp_upload_level_rows": (_c_int, [_p, _c_int, _c_int, _c_int, _p]),
    "gdp_upload_pyramid_rows": (_c_int, [_p, _c_int, _p]),
    "gdp_upload_image_raw": (_c_int, [_p, _c_int, _p]),
    "gdp_packed_floats": (_c_size, [_p]),
    "gdp_set_output_device": (_c_int, [_p, _p, _c_size]),
    "gdp_level_offset": (_c_size, [_p, _c_int, _c_int, _c_int]),
    "gdp_host_alloc": (_c_int, [_c_size, _pp]),
    "gdp_host_free": (None, [_p]),
    "gdp_image_floats": (_c_size, [_p]),
    "gdp_download_image_raw": (_c_int, [_p, _c_int, _p]),
    "gdp_generate_dog_mirrored": (_c_int, [_p, _c_int, _p]),
    "gdp_host_alloc_tracked": (_c_int, [_c_size, _pp]),
    "gdp_host_track": (_c_int, [_p, _c_size]),
    "gdp_host_untrack": (_c_int, [_p]),
    "gdp_host_arm": (_c_int, [_p]),
    "gdp_host_written_bytes": (_c_int, [_p, ctypes.POINTER(ctypes.c_size_t)]),
    "gdp_host_defer": (_c_int, [_p, _c_int, _p]),
    "gdp_host_fetch": (_c_int, [_p]),
    "gdp_host_deferred_stats": (_c_int, [_p, ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_size_t),
                                         ctypes.POINTER(ctypes.c_uint64)]),
    "gdp_upload_image_written": (_c_int, [_p, _c_int, _p]),
    "gdp_generate_dog_mirrored_written": (_c_int, [_p, _c_int, _p]),
    "gdp_set_keypoint_capacity": (_c_int, [_p, _c_size]),
    "gdp_detect_extrema": (_c_int, [_p, ctypes.c_float, ctypes.c_float, _p]),
    "gdp_keypoint_count": (_c_int, [_p, _c_int, ctypes.POINTER(_c_size)]),
    "gdp_download_keypoints": (_c_int, [_p, _c_int, _p, _c_size, ctypes.POINTER(_c_size), ctypes.POINTER(_c_size)]),
    "gdp_device_keypoints": (_c_int, [_p, _c_int, _pp, _pp]),
    "gdp_refine_keypoints": (_c_int, [_p, ctypes.c_float, ctypes.c_float, _p]),
    "gdp_refined_count": (_c_int, [_p, _c_int, ctypes.POINTER(_c_size)]),
    "gdp_download_refined": (_c_int, [_p, _c_int, _p, _c_size, ctypes.POINTER(_c_size)]),
    "gdp_device_refined": (_c_int, [_p, _c_int, _pp, _pp]),
    "gdp_upload_keypoints": (_c_int, [_p, _c_int, _p, _c_size]),
    "gdp_orient_create": (_c_int, [_pp, _p, _c_size]),
    "gdp_orient_destroy": (None, [_p]),
    "gdp_orient_last_error": (ctypes.c_char_p, [_p]),
    "gdp_orient_set_input": (_c_int, [_p, _c_int, _p, _c_size]),
    "gdp_orient_keypoints": (_c_int, [_p, _p]),
    "gdp_oriented_count": (_c_int, [_p, _c_int, ctypes.POINTER(_c_size)]),
    "gdp_download_oriented": (_c_int, [_p, _c_int, _p, _c_size, ctypes.POINTER(_c_size), ctypes.POINTER(_c_size)]),
    "gdp_device_oriented": (_c_int, [_p, _c_int, _pp, _pp]),
    "gdp_orient_weights": (_c_int, [_c_int, _c_int, _p, ctypes.POINTER(_c_int)]),
    "gdp_describe_create": (_c_int, [_pp, _p, _p, _c_size]),
    "gdp_describe_destroy": (None, [_p]),
    "gdp_describe_last_error": (ctypes.c_char_p, [_p]),
    "gdp_describe_set_input": (_c_int, [_p, _c_int, _p, _c_size]),
    "gdp_describe_keypoints": (_c_int, [_p, _p]),
    "gdp_described_count": (_c_int, [_p, _c_int, ctypes.POINTER(_c_size)]),
    "gdp_download_described": (_c_int, [_p, _c_int, _p, _c_size, ctypes.POINTER(_c_size), ctypes.POINTER(_c_size)]),
    "gdp_device_described": (_c_int, [_p, _c_int, _pp, _pp]),
    "gdp_describe_tables": (_c_int, [_c_int, _c_int, _p, ctypes.POINTER(_c_int), _p, _p]),
    "gdp_match_create": (_c_int, [_pp, _p, _p, _c_size, _c_size]),
    "gdp_match_destroy": (None, [_p]),
    "gdp_match_last_error": (ctypes.c_char_p, [_p]),
    "gdp_match_set_input": (_c_int, [_p, _c_int, _p, _c_size]),
    "gdp_match_descriptors": (_c_int, [_p, _c_int, _c_int, ctypes.c_float, _c_u32, _c_int, _p]),
    "gdp_match_count": (_c_int, [_p, ctypes.POINTER(_c_size)]),
    "gdp_download_matches": (_c_int, [_p, _p, _c_size, ctypes.POINTER(_c_size), ctypes.POINTER(_c_size)]),
    "gdp_device_matches": (_c_int, [_p, _pp, _pp]),
    "gdp_match_layout": (_c_int, [_p, ctypes.POINTER(_c_size), ctypes.POINTER(_c_size), ctypes.POINTER(_c_u32),
                                  ctypes.POINTER(_c_u32), ctypes.POINTER(_c_u32)]),
    "gdp_ransac_create": (_c_int, [_pp, _p, _c_size, _c_u32]),
    "gdp_ransac_destroy": (None, [_p]),
    "gdp_ransac_last_error": (ctypes.c_char_p, [_p]),
    "gdp_ransac_set_input": (_c_int, [_p, _p, _c_size]),
    "gdp_fit_homography": (_c_int, [_p, _c_u32, _c_u32, ctypes.c_float, _c_u32, _p]),
    "gdp_ransac_count": (_c_int, [_p, ctypes.POINTER(_c_size)]),
    "gdp_download_homography": (_c_int, [_p, _p]),
    "gdp_download_hypotheses": (_c_int, [_p, _p, _c_size, ctypes.POINTER(_c_size)]),
    "gdp_download_inliers": (_c_int, [_p, _p, _c_size, ctypes.POINTER(_c_size), ctypes.POINTER(_c_size)]),
    "gdp_device_inliers": (_c_int, [_p, _pp, _pp, _pp]),
    "gdp_ransac_layout": (_c_int, [_p, ctypes.POINTER(_c_size), ctypes.POINTER(_c_u32), ctypes.POINTER(_c_u32),
                                   ctypes.POINTER(_c_u32)]),
    "gdp_refit_homography": (_c_int, [_p, _c_u32, ctypes.c_float, _p]),
    "gdp_download_refit": (_c_int, [_p, _p]),
    "gdp_device_refit": (_c_int, [_p, _pp]),
    "gdp_warp_create": (_c_int, [_pp, _p]),
    "gdp_warp_destroy": (None, [_p]),
    "gdp_warp_last_error": (ctypes.c_char_p, [_p]),
    "gdp_warp_set_model": (_c_int, [_p, _p]),
    "gdp_warp_image": (_c_int, [_p, _c_int, _c_int, _c_int, ctypes.c_int32, _p]),
    "gdp_download_warp_record": (_c_int, [_p, _p]),
    "gdp_download_warped": (_c_int, [_p, _p, _c_size]),
    "gdp_device_warped": (_c_int, [_p, _pp, ctypes.POINTER(_c_size), ctypes.POINTER(_c_int), ctypes.POINTER(_c_int),
                                   ctypes.POINTER(_c_int), _pp]),
    "gdp_warp_layout": (_c_int, [_p, ctypes.POINTER(_c_u32), ctypes.POINTER(_c_u32), ctypes.POINTER(_c_u32)]),
    "gdp_guided_create": (_c_int, [_pp, _p, _c_u32]),
    "gdp_guided_destroy": (None, [_p]),
    "gdp_guided_last_error": (ctypes.c_char_p, [_p]),
    "gdp_guided_set_model": (_c_int, [_p, _p]),
    "gdp_match_guided": (_c_int, [_p, _c_int, _c_int, ctypes.c_float, ctypes.c_float, _c_u32, _c_int, _p]),
    "gdp_guided_count": (_c_int, [_p, ctypes.POINTER(_c_size)]),
    "gdp_download_guided": (_c_int, [_p, _p, _c_size, ctypes.POINTER(_c_size), ctypes.POINTER(_c_size)]),
    "gdp_device_guided": (_c_int, [_p, _pp, _pp]),
    "gdp_guided_layout": (_c_int, [_p, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(_c_u32), ctypes.POINTER(_c_u32),
                                   ctypes.POINTER(_c_u32), ctypes.POINTER(_c_u32)]),
    "gdp_checksum": (_c_int, [_p, _c_int, ctypes.POINTER(ctypes.c_uint64)]),
    "gdp_get_taps": (_c_int, [_p, _c_int, _c_int, _c_int, _p]),
    "gdp_set_window_centre": (_c_int, [_p, _c_int]),
    "gdp_get_window_centre": (_c_int, [_p]),
    "gdp_copy_band": (_c_int, [_p, _c_int, _p, _c_int, _p]),
    "gdp_sync": (_c_int, [_p]),
    "gdp_stream": (_p, [_p]),
    "gdp_last_error": (ctypes.c_char_p, [_p]),
    "gdp_status_string": (ctypes.c_char_p, [_c_int]),
    "gdp_time_builds": (_c_int, [_p, _c_int, _p, ctypes.POINTER(ctypes.c_float)]),
    "gdp_set_tuning": (_c_int, [_p, _c_int, _c_int]),
    "gdp_autotune": (_c_int, [_p, _c_int, _p, ctypes.POINTER(_c_int), ctypes.POINTER(_c_int),
                              ctypes.POINTER(ctypes.c_float)]),
    "gdp_get_tuning": (_c_int, [_p, _c_int, ctypes.POINTER(_c_int)]),
    "gdp_build_variants": (_c_int, [ctypes.POINTER(_c_int), _c_int]),
}


def header_functions(path=HEADER):
    """Function names declared in include/gdp.h."""
    with open(path) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    return sorted(set(re.findall(r"\b(gdp_[a-z_0-9]+)\s*\(", text)))


def _preload_torch():
    if os.environ.get("GDP_NO_TORCH") == "1":
        return
    try:
        import torch  # noqa: F401  (shares torch's HIP runtime, see module docstring)
    except ImportError:
        pass


def lib():
    """Load libgdp.so once; raise GdpError if it is absent (no fallback exists)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise GdpError(GDP_ERR_STATE, f"{LIB_PATH} not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                                      f"or `make -C sift-parallel-optimization_amd/csrc`")
    _preload_torch()
    L = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = res, args
    if L.gdp_abi_version() != 1:
        raise GdpError(GDP_ERR_STATE, "libgdp ABI version mismatch")
    _lib = L
    return L


def build_variants():
    """The build-kernel variant ids this libgdp.so holds (the values GDP_TUNE_VARIANT accepts)."""
    L = lib()
    n = L.gdp_build_variants(None, 0)
    ids = (_c_int * n)()
    L.gdp_build_variants(ids, n)
    return list(ids)


# handle kind -> the export that holds its last error text
LAST_ERROR = {"ctx": "gdp_last_error", "orient": "gdp_orient_last_error", "describe": "gdp_describe_last_error",
              "match": "gdp_match_last_error", "ransac": "gdp_ransac_last_error", "warp": "gdp_warp_last_error",
              "guided": "gdp_guided_last_error"}


def check(status, handle=None, kind="ctx"):
    """Raise GdpError for a non-zero status.  `handle` is the object the failed call was made on, or
    None for a failed create, and `kind` names what it is (a key of LAST_ERROR; an unknown one is a
    KeyError): the message is that object's last error text, else gdp_status_string(status)."""
    last_error = LAST_ERROR[kind]
    if status != GDP_OK:
        L = lib()
        raise GdpError(status, (getattr(L, last_error)(handle) or b"").decode() or L.gdp_status_string(status).decode())
    return status
