"""Host-side mirror of the reference's pyramid interface, on top of the libgdp C ABI.

`GaussPyramid` keeps the reference class's names, argument meaning and call semantics
(GuassDePyramid.h:11-29):

    g = GaussPyramid(img, len, S)   # ctor copies img[0:len][0:len] and runs GaussPyInit (:36-58)
    g.GaussPyInit()                 # refill every level with the decimated input (:60-87)
    g.GaussFilter(o)                # window-multiply every scale of octave o in place (:106-134)
    g.GenerateDoG()                 # GaussFilter + DoG for every octave, in place (:136-149)
    g.output()                      # print scale 0 of every octave (:89-104)
    g.GaussPy[o][s][r][c]           # the pyramid (downloaded lazily from the device)

GaussPy is two-way state, as the reference's float**** is (:16; GaussFilter / GenerateDoG work
on whatever the caller left in it, :122-131, :140-146): a level the caller touched through
GaussPy[o][s] is ONE host array for the object's lifetime (like a reference row, it stays live:
a handle taken before a call reads the new contents after it, and writes through it are seen),
and it may be written any way (g.GaussPy[o][s][r][c] = v, row slices, views, ufuncs with out=).
Every mutating call first uploads each touched level whose bits differ from what the device last
gave it (an exact comparison against a snapshot; levels only read are not uploaded, so reading
GaussPy — output() included — never costs the fused GaussPyInit+GenerateDoG path), then runs,
then refreshes every touched level in place — the touched levels are views into ONE host buffer in
the device's raw layout, so when they hold at least half of the pyramid's bytes (e.g. a caller
that walks every level) the refresh is one gdp_download_image_raw instead of one blocking copy per
level; levels touched once stay in the refresh for the object's lifetime (like
reference rows, a dropped handle may still have been written).  GaussPyInit re-reads the CURRENT `data` (:80) and
overwrites host edits, as the reference's refill does.  Levels never touched cost nothing.
SyncDevice() uploads the edited levels on demand.
GaussPyramid(img, len, S, defer=True) (round 6, as the C++ classes' DeferDownload): the levels are
views of ONE write-tracked host mirror in the device layout; after a call its pages are fetched
from the device only when first touched (sequential readers get the next block ahead), and the
pages the caller writes are found by page faults — no snapshot comparison, no copy of levels the
caller does not read.  Writing such an array to a file or socket straight from its memory (tofile,
np.save, file.write) may fail with EFAULT on a page not fetched yet: copy it first (np.array(a)).

Calling GenerateDoG() twice without GaussPyInit() re-filters the pyramid exactly like the
reference's timing loop does (main.cpp:66-73).  The one behavioural difference is error
handling: the reference never reports errors (all methods return void); here a failing call
raises GdpError instead of continuing on bad state.

`PyramidContext` is the batched, stream-ordered interface (one context = `batch` images or one
row band), used by bench.py and the multi-GPU driver.
"""
import ctypes
import sys
import weakref
from collections import namedtuple

import numpy as np

from ._lib import check, lib

_i = ctypes.c_int


def _ptr(a):
    return ctypes.c_void_p(a.ctypes.data)


# struct gdp_keypoint (include/gdp.h): one 16-byte record per keypoint
KEYPOINT_DTYPE = np.dtype({"names": ["octave", "scale", "kind", "row", "col", "value"],
                           "formats": [np.uint16, np.uint8, np.int8, np.int32, np.int32, np.float32],
                           "offsets": [0, 2, 3, 4, 8, 12], "itemsize": 16})


# struct gdp_keypoint_refined (include/gdp.h): 32 bytes, the first 16 a gdp_keypoint at the final sample
REFINED_DTYPE = np.dtype({"names": ["octave", "scale", "kind", "row", "col", "value", "dscale", "drow", "dcol", "interp"],
                          "formats": [np.uint16, np.uint8, np.int8, np.int32, np.int32, np.float32, np.float32,
                                      np.float32, np.float32, np.float32],
                          "offsets": [0, 2, 3, 4, 8, 12, 16, 20, 24, 28], "itemsize": 32})


# struct gdp_keypoint_oriented (include/gdp.h): 48 bytes, the first 32 the input gdp_keypoint_refined
ORIENTED_DTYPE = np.dtype({"names": ["octave", "scale", "kind", "row", "col", "value", "dscale", "drow", "dcol", "interp",
                                     "angle", "peak", "bin", "peaks"],
                           "formats": [np.uint16, np.uint8, np.int8, np.int32, np.int32, np.float32, np.float32,
                                       np.float32, np.float32, np.float32, np.float32, np.float32, np.uint32, np.uint32],
                           "offsets": [0, 2, 3, 4, 8, 12, 16, 20, 24, 28, 32, 36, 40, 44], "itemsize": 48})


# struct gdp_keypoint_described (include/gdp.h): 176 bytes, the first 48 the input gdp_keypoint_oriented
DESCRIBED_DTYPE = np.dtype({"names": list(ORIENTED_DTYPE.names) + ["desc"],
                            "formats": [ORIENTED_DTYPE.fields[n][0] for n in ORIENTED_DTYPE.names] + [(np.uint8, (128,))],
                            "offsets": [ORIENTED_DTYPE.fields[n][1] for n in ORIENTED_DTYPE.names] + [48], "itemsize": 176})


# struct gdp_match_record (include/gdp.h): 32 bytes
MATCH_DTYPE = np.dtype({"names": ["query", "train", "distance", "second", "qx", "qy", "tx", "ty"],
                        "formats": [np.uint32, np.uint32, np.uint32, np.uint32, np.float32, np.float32, np.float32, np.float32],
                        "offsets": [0, 4, 8, 12, 16, 20, 24, 28], "itemsize": 32})

# struct gdp_homography (include/gdp.h): 64 bytes
HOMOGRAPHY_DTYPE = np.dtype({"names": ["h", "hypothesis", "inliers", "matches", "sample"],
                             "formats": [(np.float32, (9,)), np.uint32, np.uint32, np.uint32, (np.uint32, (4,))],
                             "offsets": [0, 36, 40, 44, 48], "itemsize": 64})

# struct gdp_refit_record (include/gdp.h): 96 bytes
REFIT_DTYPE = np.dtype({"names": ["rounds", "accepted", "used", "skipped", "count_before", "count_after", "status", "kq", "kt",
                                  "origin", "h", "reserved"],
                        "formats": [np.uint32] * 9 + [(np.int32, (4,)), (np.float32, (9,)), (np.uint32, (2,))],
                        "offsets": [0, 4, 8, 12, 16, 20, 24, 28, 32, 36, 52, 88], "itemsize": 96})


# struct gdp_warp_record (include/gdp.h): 64 bytes
WARP_DTYPE = np.dtype({"names": ["m", "model", "covered", "pixels", "sad", "direction", "reserved"],
                       "formats": [(np.float32, (9,)), np.uint32, np.uint32, np.uint32, np.uint64, np.uint32, np.uint32],
                       "offsets": [0, 36, 40, 44, 48, 56, 60], "itemsize": 64})

WARP_DIRECTIONS = {"train_to_query": 0, "query_to_train": 1}  # GDP_WARP_TRAIN_TO_QUERY, GDP_WARP_QUERY_TO_TRAIN


class Homography(np.ndarray):
    """One HOMOGRAPHY_DTYPE record (0-d) with `matrix`: its 3 x 3 float32 array, row-major as scored,
    or None when the record holds no model."""

    @property
    def matrix(self):
        return None if int(self["hypothesis"]) == 0xffffffff else np.array(self["h"], np.float32).reshape(3, 3)


class Keypoints(np.ndarray):
    """A KEYPOINT_DTYPE array of the stored records with `found`, the number the detection counted
    (larger than len() when the context's capacity was too small)."""

    found = 0

    def __array_finalize__(self, obj):
        self.found = getattr(obj, "found", 0)


# The six stage objects a context creates on first use, upstream first, keyed by their kind (the
# name check() reports their errors under): the create and destroy exports, whether the create takes
# the context, and the object it reads — that one is created before it and destroyed after it.
_Object = namedtuple("_Object", "create destroy takes_ctx reads")
_OBJECTS = {"orient": _Object("gdp_orient_create", "gdp_orient_destroy", True, None),
            "describe": _Object("gdp_describe_create", "gdp_describe_destroy", True, "orient"),
            "match": _Object("gdp_match_create", "gdp_match_destroy", False, "describe"),  # and the train side's
            "ransac": _Object("gdp_ransac_create", "gdp_ransac_destroy", False, "match"),
            "warp": _Object("gdp_warp_create", "gdp_warp_destroy", False, "ransac"),
            "guided": _Object("gdp_guided_create", "gdp_guided_destroy", False, "ransac")}


# The list operations every stage has, each once: `export` is called on `handle` (the context or a
# stage object of `kind`) with the leading arguments `lead`: (image,), (side,) or ().
def _count(export, handle, lead, kind):
    n = ctypes.c_size_t()
    check(getattr(lib(), export)(handle, *lead, ctypes.byref(n)), handle, kind)
    return n.value


def _download(export, handle, lead, kind, dtype, room, found=True):
    """Download into `room` records and trim to the stored ones; where the export reports `found`,
    the result is a Keypoints view that carries it."""
    out = np.zeros(room, dtype)
    tail = [ctypes.c_size_t() for _ in range(2 if found else 1)]  # stored[, found]
    check(getattr(lib(), export)(handle, *lead, _ptr(out) if out.size else None, out.size, *map(ctypes.byref, tail)),
          handle, kind)
    out = out[:tail[0].value]
    if found:
        out = out.view(Keypoints)
        out.found = tail[1].value
    return out


def _device_pointers(export, handle, lead, kind, n=2):
    """The device addresses the export gives: (records, their uint32 counter[, ...])."""
    ptrs = [ctypes.c_void_p() for _ in range(n)]
    check(getattr(lib(), export)(handle, *lead, *map(ctypes.byref, ptrs)), handle, kind)
    return tuple(p.value for p in ptrs)


def _set_list_input(export, handle, lead, kind, recs, dtype):
    """Make `recs` the stage's input list; None goes back to the list of the stage before it."""
    if recs is None:
        check(getattr(lib(), export)(handle, *lead, None, 0), handle, kind)
        return
    recs = np.ascontiguousarray(recs, dtype=dtype).reshape(-1)
    keep = recs if recs.size else np.zeros(1, dtype)  # an empty list is still a list: a non-null pointer
    check(getattr(lib(), export)(handle, *lead, _ptr(keep), recs.size), handle, kind)


GDP_STREAM_NULL = 1  # include/gdp.h: selects HIP's default (null) stream


def _stream_handle(stream):
    """None -> the context's own stream; a torch.cuda.Stream or raw int handle -> that stream
    (handle 0, torch's default stream, is passed as GDP_STREAM_NULL so it is not mistaken for
    "the context's stream")."""
    if stream is None:
        return None
    handle = stream if isinstance(stream, int) else getattr(stream, "cuda_stream", None)
    if handle is None:
        raise TypeError(f"unsupported stream object {stream!r}")
    return ctypes.c_void_p(handle if handle != 0 else GDP_STREAM_NULL)


def octaves_for(n):
    """floor(log2 n) + 1 — the reference's `layer` (GuassDePyramid.h:48-53)."""
    return lib().gdp_octaves_for(int(n))


def conv_taps(S, scale):
    """(taps[0:2R+1], R) of the convolution-mode Gaussian of `scale` (gdp_conv_taps)."""
    t = np.zeros(13, np.float32)
    r = _i()
    check(lib().gdp_conv_taps(int(S), int(scale), _ptr(t), ctypes.byref(r)))
    return t[:2 * r.value + 1].copy(), r.value


def orient_weights(S, scale):
    """(w[0:2R*R+1], R): the orientation window of `scale` in a pyramid of S — w[d2] weighs a sample
    at squared distance d2 (gdp_orient_weights)."""
    t = np.zeros(51, np.float32)
    r = _i()
    check(lib().gdp_orient_weights(int(S), int(scale), _ptr(t), ctypes.byref(r)))
    return t[:2 * r.value * r.value + 1].copy(), r.value


def describe_tables(S, scale):
    """(W[0:2R*R+1], R, C[0:1440], S[0:1440]): the descriptor window of `scale` in a pyramid of S —
    W[d2] weighs a sample at squared distance d2 — and the quarter-degree rotation table
    (gdp_describe_tables)."""
    t = np.zeros(243, np.float32)
    cos, sin = np.zeros(1440, np.float32), np.zeros(1440, np.float32)
    r = _i()
    check(lib().gdp_describe_tables(int(S), int(scale), _ptr(t), ctypes.byref(r), _ptr(cos), _ptr(sin)))
    return t[:2 * r.value * r.value + 1].copy(), r.value, cos, sin


class PyramidContext:
    """`batch` images of H x W int32 (or the row band [row_begin, row_end)) on one GPU.

    Level (o, s) of image b is a rows_o x cols_o float32 array; rows_o covers the band's rows.
    All compute calls are asynchronous on `stream` (None = the context's own stream).
    """

    def __init__(self, height, width, S=2, octaves=0, batch=1, device=0, row_begin=0, row_end=None,
                 input_format="i32", centre="serial"):
        # everything close() reads exists before the first call that can fail
        self._ctx = ctypes.c_void_p()
        self._handles = {name: ctypes.c_void_p() for name in _OBJECTS}  # the stage objects, null until first use
        self._made_from = dict.fromkeys(_OBJECTS)  # the upstream handles each was created from
        self._capacity = {"orient": (0,), "describe": (0,), "match": (0, 0), "ransac": (0, 0), "warp": (),
                          "guided": (0,)}  # create's sizes, 0: its default
        self._records = {"orient": 0, "describe": 0}  # what the object holds per image, known at creation
        self._train = None  # weak reference to the train context of the match object
        self._match_readers = weakref.WeakSet()  # the contexts whose match object reads this one's describe object
        L = lib()
        row_end = height if row_end is None else row_end
        check(L.gdp_create_band(ctypes.byref(self._ctx), int(height), int(width), int(S), int(octaves), int(batch),
                                int(row_begin), int(row_end), int(device)))
        H, W, S_, O, B = (_i() for _ in range(5))
        check(L.gdp_get_geometry(self._ctx, *(ctypes.byref(v) for v in (H, W, S_, O, B))), self._ctx)
        self.H, self.W, self.S, self.O, self.batch = H.value, W.value, S_.value, O.value, B.value
        self.device = device
        self.row_begin, self.row_end = int(row_begin), int(row_end)
        self._dims = []
        for o in range(self.O):
            r, c, f = _i(), _i(), _i()
            check(L.gdp_level_dims(self._ctx, o, ctypes.byref(r), ctypes.byref(c), ctypes.byref(f)), self._ctx)
            self._dims.append((r.value, c.value, f.value))
        self._bound = None  # keeps a caller's device input alive
        self._kp_capacity = 65536  # gdp_set_keypoint_capacity's default
        self.input_format = "i32"
        if input_format != "i32":
            self.set_input_format(input_format)
        self.centre = "serial"
        if centre != "serial":
            self.set_window_centre(centre)

    def set_window_centre(self, mode):
        """'serial' (GuassDePyramid.h:107-115: the float length halved o times) or 'intlen'
        (the multi-process variants' integer length, GaussDePyramid-MPI.h:273, mpitest.cpp:44)."""
        from ._lib import GDP_CENTRE_INTLEN, GDP_CENTRE_SERIAL

        code = {"serial": GDP_CENTRE_SERIAL, "intlen": GDP_CENTRE_INTLEN}[mode]
        check(lib().gdp_set_window_centre(self._ctx, code), self._ctx)
        self.centre = mode

    def copy_band_from(self, full, b=0, full_image=0, stream=None):
        """Load this band context's rows of `full`'s current pyramid (gdp_copy_band)."""
        check(lib().gdp_copy_band(self._ctx, int(b), full._ctx, int(full_image), _stream_handle(stream)), self._ctx)

    def set_input_format(self, fmt):
        """'i32' (the reference's int pixels) or 'u8' (8-bit images, 4x fewer input bytes)."""
        from ._lib import GDP_INPUT_I32, GDP_INPUT_U8

        code = {"i32": GDP_INPUT_I32, "u8": GDP_INPUT_U8}[fmt]
        check(lib().gdp_set_input_format(self._ctx, code), self._ctx)
        self.input_format = fmt

    # ------------------------------------------------------------------ geometry
    @property
    def levels_per_octave(self):
        return self.S + 3

    def level_dims(self, o):
        """(rows held, cols, first global row) of octave o."""
        return self._dims[o]

    def packed_floats(self):
        return lib().gdp_packed_floats(self._ctx)

    def pyramid_bytes(self):
        return lib().gdp_pyramid_bytes(self._ctx)

    # ------------------------------------------------------------------ input
    def set_input(self, img, b=0, stream=None):
        """Upload one H x W (band: band-rows x W) image from host memory, in the context's input
        format (int32, or uint8 for an input_format='u8' context)."""
        u8 = self.input_format == "u8"
        img = np.asarray(img)
        if u8 and img.dtype != np.uint8:
            raise TypeError("a u8 context takes uint8 images")
        img = np.ascontiguousarray(img, dtype=np.uint8 if u8 else np.int32)
        rows = self.row_end - self.row_begin
        if img.ndim != 2 or img.shape[1] != self.W or img.shape[0] != rows:
            raise ValueError(f"expected a ({rows}, {self.W}) image, got {img.shape}")
        fn = lib().gdp_set_input_host_u8 if u8 else lib().gdp_set_input_host
        check(fn(self._ctx, int(b), _ptr(img), self.W, _stream_handle(stream)), self._ctx)

    def set_input_rows(self, rows, b=0, stream=None):
        """Upload from a list of row arrays — the reference ctor's `int** img` (GuassDePyramid.h:38-46)."""
        arrs = [np.ascontiguousarray(r, dtype=np.int32) for r in rows]
        ptrs = (ctypes.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])
        check(lib().gdp_set_input_rows(self._ctx, int(b), ptrs, _stream_handle(stream)), self._ctx)

    def bind_device_input(self, ptr, pitch, image_stride, keepalive=None):
        """Read images straight from caller device memory (pitch/stride in elements of the
        context's input format)."""
        fn = lib().gdp_set_input_device_u8 if self.input_format == "u8" else lib().gdp_set_input_device
        check(fn(self._ctx, ctypes.c_void_p(ptr), int(pitch), int(image_stride)), self._ctx)
        self._bound = keepalive

    def unbind_device_input(self):
        check(lib().gdp_set_input_device(self._ctx, None, 0, 0), self._ctx)
        self._bound = None

    # ------------------------------------------------------------------ row-band halos (conv extension)
    def conv_halo_rows(self):
        """(above, below): input rows a band's build_gaussian reads beyond its own rows."""
        a, b = _i(), _i()
        check(lib().gdp_conv_halo_rows(self._ctx, ctypes.byref(a), ctypes.byref(b)), self._ctx)
        return a.value, b.value

    def bind_input_halo(self, above=None, below=None, pitch=None, image_stride=None, keepalive=None):
        """Read the halo rows from caller device memory (device pointers, [batch][rows][pitch] in
        the input format; pitch defaults to the width)."""
        pitch = self.W if pitch is None else int(pitch)
        na, nb = self.conv_halo_rows()
        stride = pitch * max(na, nb, 1) if image_stride is None else int(image_stride)
        check(lib().gdp_bind_input_halo(self._ctx, ctypes.c_void_p(above or 0) if above else None,
                                        ctypes.c_void_p(below or 0) if below else None, pitch, stride), self._ctx)
        self._halo_keepalive = keepalive

    def input_halo(self, side):
        """(device address, pitch) of the context's own halo buffer (side 0 above, 1 below),
        allocated on first call and used by the next band builds; (None, pitch) when none is needed."""
        ptr, pitch = ctypes.c_void_p(), ctypes.c_size_t()
        check(lib().gdp_input_halo(self._ctx, int(side), ctypes.byref(ptr), ctypes.byref(pitch)), self._ctx)
        return ptr.value, pitch.value

    def device_input(self, b=0):
        """(device address, pitch) of image b's input rows (own buffer or the bound one)."""
        ptr, pitch = ctypes.c_void_p(), ctypes.c_size_t()
        check(lib().gdp_device_input(self._ctx, int(b), ctypes.byref(ptr), ctypes.byref(pitch)), self._ctx)
        return ptr.value, pitch.value

    def fill_synthetic(self, seed=0x5EED, first_image=0, stream=None):
        check(lib().gdp_fill_synthetic(self._ctx, int(seed) & 0xFFFFFFFF, int(first_image), _stream_handle(stream)),
              self._ctx)

    # ------------------------------------------------------------------ compute
    def build(self, stream=None):
        """Fused GaussPyInit + GenerateDoG of every image (one launch)."""
        check(lib().gdp_build(self._ctx, _stream_handle(stream)), self._ctx)

    def build_gaussian(self, stream=None):
        """Extension (no reference counterpart): true separable Gaussian convolution pyramid."""
        check(lib().gdp_build_gaussian(self._ctx, _stream_handle(stream)), self._ctx)

    def init(self, stream=None):
        check(lib().gdp_init(self._ctx, _stream_handle(stream)), self._ctx)

    def gauss_octave(self, o, stream=None):
        check(lib().gdp_gauss_octave(self._ctx, int(o), _stream_handle(stream)), self._ctx)

    def gauss_range(self, o_begin=0, o_end=None, stream=None):
        """GaussFilter of octaves [o_begin, o_end) in one launch (in place)."""
        o_end = self.O if o_end is None else o_end
        check(lib().gdp_gauss_range(self._ctx, int(o_begin), int(o_end), _stream_handle(stream)), self._ctx)

    def gauss_scales(self, s_begin, s_end, o_begin=0, o_end=None, stream=None):
        """Window multiply of scales [s_begin, s_end) of octaves [o_begin, o_end) in place (the MPI
        variant's worker step, GaussDePyramid-MPI.h:271-290)."""
        o_end = self.O if o_end is None else o_end
        check(lib().gdp_gauss_scales(self._ctx, int(s_begin), int(s_end), int(o_begin), int(o_end),
                                     _stream_handle(stream)), self._ctx)

    def dog_octave(self, o, stream=None):
        check(lib().gdp_dog_octave(self._ctx, int(o), _stream_handle(stream)), self._ctx)

    def dog_range(self, o_begin=0, o_end=None, stream=None):
        """The DoG pass of octaves [o_begin, o_end) in one launch."""
        o_end = self.O if o_end is None else o_end
        check(lib().gdp_dog_range(self._ctx, int(o_begin), int(o_end), _stream_handle(stream)), self._ctx)

    def generate_dog(self, stream=None):
        check(lib().gdp_generate_dog(self._ctx, _stream_handle(stream)), self._ctx)

    def build_subset(self, stream=None):
        """Fused GaussPyInit + GaussPyramid_a512omp::GenerateDoG_nomp_dynamic (the AVX-512 x OpenMP
        header's subset: scales 0..S-1 windowed, DoG for s < S-1; see gdp.h)."""
        check(lib().gdp_build_subset(self._ctx, _stream_handle(stream)), self._ctx)

    def generate_dog_subset(self, stream=None):
        """GenerateDoG_nomp_dynamic in place on the current contents."""
        check(lib().gdp_generate_dog_subset(self._ctx, _stream_handle(stream)), self._ctx)

    def sync(self):
        check(lib().gdp_sync(self._ctx), self._ctx)

    @property
    def stream(self):
        return lib().gdp_stream(self._ctx)

    _TUNING = ("nontemporal", "blocks_per_cu", "grid", "variant", "tile_order", "inplace_sub", "window_sub",
               "conv_kernel", "conv_rows", "conv_order", "build_lds", "stage_kb", "stage_threads", "conv_waves", "zero_window",
               "store_pace", "conv_pace", "inplace_pace", "keep_zeros", "keep_kernel", "keep_signs", "keep_support",
               "pyramid_chunk_kb", "zeros_clean", "signs_known", "keep_signs_kernel",
               "keep_support_units")  # the last five read-only

    @staticmethod
    def _tuning_key(name):
        from . import _lib

        return getattr(_lib, "GDP_TUNE_" + name.upper())

    def set_tuning(self, nontemporal=None, blocks_per_cu=None, grid=None, variant=None, tile_order=None,
                   inplace_sub=None, window_sub=None, conv_kernel=None, conv_rows=None, conv_order=None,
                   build_lds=None, stage_kb=None, stage_threads=None, conv_waves=None, zero_window=None,
                   store_pace=None, conv_pace=None, inplace_pace=None, keep_zeros=None,
                   keep_kernel=None, keep_signs=None, keep_support=None):
        """Performance knobs of the kernels (outputs are bit-identical for every setting; the
        conv_* knobs select the convolution extension's kernel: 0 register sweep, 1 LDS tiles,
        2 block tiles, and the sweep's rows per wave strip (16 / 32) or the block tiles' rows per
        block with conv_waves waves per block (16 waves: 16 / 32 / 48 rows; 8 waves: 8 / 16 / 24 /
        32 rows — any other pair makes build_gaussian raise GdpError); stage_kb / stage_threads
        size the double-buffered pinned staging of the row-pointer downloads; zero_window = 1 lets the
        build store the input-independent levels of pixels outside every window's support without
        waiting for their input; store_pace / conv_pace / inplace_pace pace the stores of the
        builds / the convolution block tiles / the in-place re-entry, each its own field;
        keep_zeros = 0 makes every build store every byte, instead of leaving the input-independent
        zeros outside the windows' support that the previous build of this context already stored —
        tuning()["zeros_clean"] tells whether the next build may leave them; keep_kernel picks the
        kernel of such a build: 0 the build kernel's own keep path, 1 / 2 the steady-state kernel with
        4 / 2 rows per wave, taken where the width is a multiple of 4; keep_signs = 0 makes every
        such build store all of level S+2 = copysign(0, x), instead of skipping the tile rows that
        held no negative int32 pixel at this build and the one before —
        tuning()["signs_known"] tells whether the next one may skip; keep_support = 0 makes the
        steady-state kernel run the groups inside the windows' support in their tiles' blocks instead
        of as work units of their own — tuning()["keep_support_units"] counts them)."""
        vals = dict(nontemporal=nontemporal, blocks_per_cu=blocks_per_cu, grid=grid, variant=variant,
                    tile_order=tile_order, inplace_sub=inplace_sub, window_sub=window_sub, conv_kernel=conv_kernel,
                    conv_rows=conv_rows, conv_order=conv_order, build_lds=build_lds, stage_kb=stage_kb,
                    stage_threads=stage_threads, conv_waves=conv_waves, zero_window=zero_window,
                    store_pace=store_pace, conv_pace=conv_pace, inplace_pace=inplace_pace, keep_zeros=keep_zeros,
                    keep_kernel=keep_kernel, keep_signs=keep_signs, keep_support=keep_support)
        for name, val in vals.items():
            if val is not None:
                check(lib().gdp_set_tuning(self._ctx, self._tuning_key(name), int(val)), self._ctx)

    def autotune(self, iters=5, stream=None):
        """Time every build variant x tile order x store mode (zero_window, store_pace) on the
        current input and keep the fastest;
        returns (variant, tile_order, ms per build).  Overwrites the pyramid (bits unchanged)."""
        v, o, ms = _i(), _i(), ctypes.c_float()
        check(lib().gdp_autotune(self._ctx, int(iters), _stream_handle(stream), ctypes.byref(v), ctypes.byref(o),
                                 ctypes.byref(ms)), self._ctx)
        return v.value, o.value, ms.value

    def tuning(self):
        """Current value of every knob of set_tuning()."""
        out = {}
        for name in self._TUNING:
            v = _i()
            check(lib().gdp_get_tuning(self._ctx, self._tuning_key(name), ctypes.byref(v)), self._ctx)
            out[name] = v.value
        return out

    def time_builds(self, iters, stream=None):
        """Total ms of `iters` back-to-back builds, HIP events on the launch stream."""
        ms = ctypes.c_float()
        check(lib().gdp_time_builds(self._ctx, int(iters), _stream_handle(stream), ctypes.byref(ms)), self._ctx)
        return ms.value

    # ------------------------------------------------------------------ output
    def level(self, b, o, s):
        rows, cols, _ = self._dims[o]
        out = np.empty((rows, cols), np.float32)
        if out.size:
            check(lib().gdp_download_level(self._ctx, int(b), int(o), int(s), _ptr(out)), self._ctx)
        return out

    def level_range(self, b, o, s, first_row, nrows):
        """Rows [first_row, first_row + nrows) of level (o, s) of image b, without downloading the
        whole level."""
        cols = self._dims[o][1]
        out = np.empty((int(nrows), cols), np.float32)
        check(lib().gdp_download_level_range(self._ctx, int(b), int(o), int(s), int(first_row), int(nrows),
                                             _ptr(out)), self._ctx)
        return out

    def level_rows(self, b, o, s, rows_out):
        """Download into a list of preallocated float32 row arrays (float**** materialisation)."""
        ptrs = (ctypes.c_void_p * len(rows_out))(*[r.ctypes.data for r in rows_out])
        check(lib().gdp_download_level_rows(self._ctx, int(b), int(o), int(s), ptrs), self._ctx)

    def pyramid(self, b=0):
        """Packed [o][s][rows][cols] float32 copy of image b's pyramid."""
        out = np.empty(self.packed_floats(), np.float32)
        check(lib().gdp_download_pyramid(self._ctx, int(b), _ptr(out)), self._ctx)
        return out

    def upload_level(self, b, o, s, arr):
        """Copy a dense rows x cols float32 host array into level (o, s) of image b."""
        rows, cols, _ = self._dims[o]
        arr = np.ascontiguousarray(arr, dtype=np.float32)
        if arr.shape != (rows, cols):
            raise ValueError(f"level ({o}, {s}) is {rows} x {cols}, got {arr.shape}")
        if arr.size:
            check(lib().gdp_upload_level(self._ctx, int(b), int(o), int(s), _ptr(arr)), self._ctx)

    def upload_pyramid(self, packed, b=0):
        packed = np.ascontiguousarray(packed, dtype=np.float32)
        if packed.size != self.packed_floats():
            raise ValueError("packed pyramid has the wrong size")
        check(lib().gdp_upload_pyramid(self._ctx, int(b), _ptr(packed)), self._ctx)

    def levels(self, b=0):
        """{(o, s): 2-D array} of image b."""
        return {(o, s): self.level(b, o, s) for o in range(self.O) for s in range(self.S + 3)}

    def bind_device_output(self, ptr, nbytes, keepalive=None):
        """Write pyramids into caller device memory (>= pyramid_bytes(), 256-B aligned)."""
        check(lib().gdp_set_output_device(self._ctx, ctypes.c_void_p(ptr), int(nbytes)), self._ctx)
        self._out_bound = keepalive

    def unbind_device_output(self):
        check(lib().gdp_set_output_device(self._ctx, None, 0), self._ctx)
        self._out_bound = None

    def level_offset(self, b, o, s):
        """Float offset of level (o, s) of image b inside the (bound or own) pyramid buffer."""
        return lib().gdp_level_offset(self._ctx, int(b), int(o), int(s))

    def checksum(self, b=0):
        """Order-independent 64-bit checksum of image b's pyramid (see gdp.h)."""
        v = ctypes.c_uint64()
        check(lib().gdp_checksum(self._ctx, int(b), ctypes.byref(v)), self._ctx)
        return v.value

    # ------------------------------------------------------------------ the stage objects (_OBJECTS)
    def _readers(self, name):
        """(context, object) of everything that reads this context's `name` object: the objects made
        from it here and, for the describe object, the match objects of the contexts that match
        against this one as their train side."""
        for reader, entry in _OBJECTS.items():
            if entry.reads == name:
                yield self, reader
        if name == "describe":
            for other in list(self._match_readers):
                yield other, "match"

    def _drop(self, name):
        """Destroy the `name` object and, first, everything that reads it."""
        for ctx, reader in self._readers(name):
            ctx._drop(reader)
        if self._handles[name].value:
            getattr(lib(), _OBJECTS[name].destroy)(self._handles[name])
            self._handles[name] = ctypes.c_void_p()

    def _handle(self, name, train=None):
        """The `name` object, created on first use from the objects it reads (themselves created on
        first use) and again whenever one of those was.  The match object reads this context's
        describe object and `train`'s (None: the train side it was last made against, or this
        context's); it is made again when `train` changes, and holds `train` only weakly."""
        entry = _OBJECTS[name]
        if name == "match":
            kept = self._train() if self._handles["match"].value else None
            if train is None:
                train = self if kept is None else kept
            if train is not kept:
                self._drop("match")  # before anything of the new train side is created
        src = ((self._ctx,) if entry.takes_ctx else ()) + ((self._handle(entry.reads),) if entry.reads else ())
        if name == "match":
            src += (train._handle("describe"),)
        made_from = tuple(s.value for s in src)
        if not self._handles[name].value or self._made_from[name] != made_from:
            self._drop(name)
            new = ctypes.c_void_p()
            check(getattr(lib(), entry.create)(ctypes.byref(new), *src, *self._capacity[name]), None, name)
            self._handles[name], self._made_from[name] = new, made_from
            if name == "orient":
                self._records[name] = self._capacity[name][0] or 2 * self._kp_capacity
            elif name == "describe":
                self._records[name] = self._capacity[name][0] or self._records["orient"]
            elif name == "match":
                self._train = weakref.ref(train)
                train._match_readers.add(self)
        return self._handles[name]

    # the names the stage tests reach the objects by: the handles as they are (null before first use),
    # and the warp object created on first use
    _orient, _describe, _match, _ransac = (property(lambda self, name=name: self._handles[name])
                                           for name in ("orient", "describe", "match", "ransac"))

    def _warp_handle(self):
        return self._handle("warp")

    def _set_model(self, name, h):
        """set_warp_model and set_guided_model: nine floats, or None, to the `name` object's gdp_<name>_set_model."""
        obj = self._handle(name)
        if h is not None:
            h = np.ascontiguousarray(h, dtype=np.float32).reshape(-1)
            if h.size != 9:
                raise ValueError(f"a {name} model is nine floats")
        check(getattr(lib(), f"gdp_{name}_set_model")(obj, None if h is None else _ptr(h)), obj, name)

    def _set_capacity(self, name, capacity):
        self._drop(name)  # the next use creates it again, of the new size
        self._capacity[name] = capacity

    # ------------------------------------------------------------------ keypoints (extension)
    def set_keypoint_capacity(self, n):
        """Records kept per image by detect_extrema (default 65536); reallocates the buffer."""
        check(lib().gdp_set_keypoint_capacity(self._ctx, int(n)), self._ctx)
        self._kp_capacity = int(n)

    def detect_extrema(self, contrast=0.0, edge_ratio=0.0, stream=None):
        """Find the strict scale-space extrema of the CURRENT pyramid's levels 0..S+1 on the device
        (gdp_detect_extrema: |value| > contrast, and the edge test when edge_ratio != 0);
        asynchronous on `stream`, one launch for every image and octave."""
        check(lib().gdp_detect_extrema(self._ctx, float(contrast), float(edge_ratio), _stream_handle(stream)),
              self._ctx)

    def keypoint_count(self, b=0):
        """Keypoints the last detection found in image b (blocking; may exceed the capacity)."""
        return _count("gdp_keypoint_count", self._ctx, (int(b),), "ctx")

    def keypoints(self, b=0):
        """The stored records of image b as a KEYPOINT_DTYPE array sorted by (octave, scale, row,
        col) (blocking); its `found` attribute is keypoint_count(b)."""
        return _download("gdp_download_keypoints", self._ctx, (int(b),), "ctx", KEYPOINT_DTYPE,
                         min(self.keypoint_count(b), self._kp_capacity))

    def device_keypoints(self, b=0):
        """(device address of image b's records, device address of its uint32 counter)."""
        return _device_pointers("gdp_device_keypoints", self._ctx, (int(b),), "ctx")

    def refine_keypoints(self, contrast=0.0, edge_ratio=0.0, stream=None):
        """Localise image by image the records of the keypoint list (the last detect_extrema's, or
        upload_keypoints') to sub-sample precision on the CURRENT pyramid (gdp_refine_keypoints:
        quadratic fit, at most 5 moves, |interp| > contrast, and the edge test when edge_ratio
        != 0); asynchronous on `stream`, one launch, no host read of the counter."""
        check(lib().gdp_refine_keypoints(self._ctx, float(contrast), float(edge_ratio), _stream_handle(stream)),
              self._ctx)

    def refined_count(self, b=0):
        """Records the last refinement kept in image b (blocking)."""
        return _count("gdp_refined_count", self._ctx, (int(b),), "ctx")

    def refined_keypoints(self, b=0):
        """The refined records of image b as a REFINED_DTYPE array sorted by (octave, scale, row,
        col) and then by the bits of the other fields (blocking)."""
        return _download("gdp_download_refined", self._ctx, (int(b),), "ctx", REFINED_DTYPE, self.refined_count(b), found=False)

    def device_refined(self, b=0):
        """(device address of image b's refined records, device address of its uint32 counter)."""
        return _device_pointers("gdp_device_refined", self._ctx, (int(b),), "ctx")

    def upload_keypoints(self, records, b=0):
        """Make `records` (KEYPOINT_DTYPE, or anything numpy converts to it) image b's keypoint
        list (blocking; gdp_upload_keypoints validates every record)."""
        recs = np.ascontiguousarray(records, dtype=KEYPOINT_DTYPE).reshape(-1)
        check(lib().gdp_upload_keypoints(self._ctx, int(b), _ptr(recs) if recs.size else None, recs.size), self._ctx)

    # ------------------------------------------------------------------ orientation (extension)
    # The gdp_orient object only reads the context: no call below changes the pyramid or the lists.
    def set_orient_capacity(self, n):
        """Oriented records kept per image, and the longest list set_orient_input takes (default:
        twice the keypoint capacity when the first orientation call is made).  Drops the earlier
        results and input lists."""
        if int(n) <= 0:
            raise ValueError("the orientation capacity must be > 0")
        self._set_capacity("orient", (int(n),))

    def set_orient_input(self, recs, b=0):
        """Make `recs` (REFINED_DTYPE, or anything numpy converts to it) image b's orientation input
        instead of the context's refined list (blocking; gdp_orient_set_input validates every
        record); None goes back to the refined list."""
        _set_list_input("gdp_orient_set_input", self._handle("orient"), (int(b),), "orient", recs, REFINED_DTYPE)

    def orient_keypoints(self, stream=None):
        """Assign orientations to every image's refined list (the last refine_keypoints', or
        set_orient_input's) on the CURRENT pyramid (gdp_orient_keypoints: the Gaussian level rebuilt
        from levels s..S+2, a 36-bin gradient histogram, one record per peak); asynchronous on
        `stream`, one launch, no host read of the counter."""
        w = self._handle("orient")
        check(lib().gdp_orient_keypoints(w, _stream_handle(stream)), w, "orient")

    def oriented_count(self, b=0):
        """Records the last orientation produced for image b (blocking; may exceed the capacity)."""
        w = self._handles["orient"]
        return _count("gdp_oriented_count", w, (int(b),), "orient") if w.value else 0

    def oriented_keypoints(self, b=0):
        """The stored records of image b as an ORIENTED_DTYPE array sorted by (octave, scale, row,
        col, bin) and then by the records' words (blocking); its `found` attribute is
        oriented_count(b)."""
        w = self._handles["orient"]
        if not w.value:
            return np.zeros(0, ORIENTED_DTYPE).view(Keypoints)
        return _download("gdp_download_oriented", w, (int(b),), "orient", ORIENTED_DTYPE,
                         min(self.oriented_count(b), self._records["orient"]))

    def device_oriented(self, b=0):
        """(device address of image b's oriented records, device address of its uint32 counter)."""
        return _device_pointers("gdp_device_oriented", self._handle("orient"), (int(b),), "orient")

    # ------------------------------------------------------------------ descriptors (extension)
    # The gdp_describe object only reads the context and its orientation object: no call below changes
    # the pyramid or any of the three lists.
    def set_describe_capacity(self, n):
        """Described records kept per image, and the longest list set_describe_input takes (default:
        the orientation capacity when the first descriptor call is made).  Drops the earlier results
        and input lists."""
        if int(n) <= 0:
            raise ValueError("the descriptor capacity must be > 0")
        self._set_capacity("describe", (int(n),))

    def set_describe_input(self, recs, b=0):
        """Make `recs` (ORIENTED_DTYPE, or anything numpy converts to it) image b's descriptor input
        instead of the oriented list (blocking; gdp_describe_set_input validates every record, the
        angle's range included); None goes back to the oriented list."""
        _set_list_input("gdp_describe_set_input", self._handle("describe"), (int(b),), "describe", recs, ORIENTED_DTYPE)

    def describe_keypoints(self, stream=None):
        """Compute the 128-byte SIFT descriptor of every image's oriented list (the last
        orient_keypoints', or set_describe_input's) on the CURRENT pyramid (gdp_describe_keypoints:
        the Gaussian level rebuilt from levels s..S+2, a rotated 4 x 4 x 8 gradient histogram,
        normalised, clipped at 0.2 and quantised); asynchronous on `stream`, one launch, no host read
        of the counter."""
        w = self._handle("describe")
        check(lib().gdp_describe_keypoints(w, _stream_handle(stream)), w, "describe")

    def described_count(self, b=0):
        """Records the last description produced for image b (blocking; may exceed the capacity)."""
        w = self._handles["describe"]
        return _count("gdp_described_count", w, (int(b),), "describe") if w.value else 0

    def described_keypoints(self, b=0):
        """The stored records of image b as a DESCRIBED_DTYPE array sorted by (octave, scale, row,
        col, bin) and then by the records' words (blocking); its `found` attribute is
        described_count(b)."""
        w = self._handles["describe"]
        if not w.value:
            return np.zeros(0, DESCRIBED_DTYPE).view(Keypoints)
        return _download("gdp_download_described", w, (int(b),), "describe", DESCRIBED_DTYPE,
                         min(self.described_count(b), self._records["describe"]))

    def device_described(self, b=0):
        """(device address of image b's described records, device address of its uint32 counter)."""
        return _device_pointers("gdp_device_described", self._handle("describe"), (int(b),), "describe")

    # ------------------------------------------------------------------ descriptor matching (extension)
    # The gdp_match object only reads the two describe objects.
    def set_match_capacity(self, query=0, train=0):
        """Records the match object holds per side (0: that side's descriptor capacity); the query
        capacity is also the most matches kept.  Drops the earlier results and input lists."""
        if int(query) < 0 or int(train) < 0:
            raise ValueError("a match capacity must be >= 0")
        self._set_capacity("match", (int(query), int(train)))

    def match_descriptors(self, train=None, query_image=0, train_image=0, ratio=0.8, max_distance=None, mutual=False, stream=None):
        """Match image `query_image`'s described list of this context against image `train_image`'s
        of `train` (another PyramidContext on the same device, None: this one) on the device
        (gdp_match_descriptors: exact nearest and second-nearest by squared L2 distance on the i8
        matrix cores, ties to the lowest index; Lowe's ratio test with `ratio` (0: off), a distance
        cap and the mutual test); asynchronous on `stream`, no host read of either counter."""
        m = self._handle("match", self if train is None else train)
        cap = 0xffffffff if max_distance is None else int(max_distance)
        check(lib().gdp_match_descriptors(m, int(query_image), int(train_image), float(ratio), cap, int(bool(mutual)),
                                          _stream_handle(stream)), m, "match")

    def set_match_input(self, side, recs):
        """Make `recs` (DESCRIBED_DTYPE) the list of `side` (0 query, 1 train) instead of the
        describe object's (blocking; records are not validated: any 176 bytes are a record); None
        goes back to the describe object's list."""
        _set_list_input("gdp_match_set_input", self._handle("match"), (int(side),), "match", recs, DESCRIBED_DTYPE)

    def match_count(self):
        """Records the last match produced (blocking; 0 before any)."""
        m = self._handles["match"]
        return _count("gdp_match_count", m, (), "match") if m.value else 0

    def matches(self):
        """The last match's records as a MATCH_DTYPE array sorted by `query` (blocking); its `found`
        attribute is match_count()."""
        m = self._handles["match"]
        if not m.value:
            return np.zeros(0, MATCH_DTYPE).view(Keypoints)
        return _download("gdp_download_matches", m, (), "match", MATCH_DTYPE, self.match_count())

    def device_matches(self):
        """(device address of the match records, device address of their uint32 counter)."""
        return _device_pointers("gdp_device_matches", self._handle("match"), (), "match")

    def match_layout(self):
        """(query capacity, train capacity, chunk granule, train chunks, query chunks) of the match
        object (gdp_match_layout)."""
        m = self._handle("match")
        qc, tc = ctypes.c_size_t(), ctypes.c_size_t()
        unit, tch, qch = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
        check(lib().gdp_match_layout(m, ctypes.byref(qc), ctypes.byref(tc), ctypes.byref(unit), ctypes.byref(tch), ctypes.byref(qch)),
              m, "match")
        return qc.value, tc.value, unit.value, tch.value, qch.value

    # ------------------------------------------------------------------ RANSAC homography (extension)
    def set_ransac_capacity(self, n=0, max_hypotheses=0):
        """The longest list a fit reads, which is also the most inliers kept (0: the match object's
        query capacity), and the most hypotheses of one fit (0: 4,096; at most 65,536).  Drops the
        earlier results and the input list."""
        if int(n) < 0 or int(max_hypotheses) < 0:
            raise ValueError("a RANSAC capacity must be >= 0")
        self._set_capacity("ransac", (int(n), int(max_hypotheses)))

    def fit_homography(self, hypotheses=1024, seed=0, threshold=3.0, min_inliers=4, stream=None):
        """Fit a homography to the last match's records (or set_ransac_input's) on the device
        (gdp_fit_homography: `hypotheses` four-point homographies in float64 without a division,
        each scored in float32 against every match with the transfer error `threshold` in pixels,
        the largest count wins, ties to the lowest index); asynchronous on `stream`, no host read of
        the match counter."""
        r = self._handle("ransac")
        check(lib().gdp_fit_homography(r, int(hypotheses), int(seed) & 0xffffffff, float(threshold), int(min_inliers),
                                       _stream_handle(stream)), r, "ransac")

    def set_ransac_input(self, recs):
        """Make `recs` (MATCH_DTYPE) the list a fit reads instead of the match object's (blocking;
        records are not validated: any 32 bytes are a record); None goes back to the match object's."""
        _set_list_input("gdp_ransac_set_input", self._handle("ransac"), (), "ransac", recs, MATCH_DTYPE)

    def homography(self):
        """The last fit's model record (blocking) as a Homography: its `matrix` is the 3 x 3 float32
        array, or None when there is no model (hypothesis = 0xffffffff)."""
        r = self._handle("ransac")
        out = np.zeros(1, HOMOGRAPHY_DTYPE)
        check(lib().gdp_download_homography(r, _ptr(out)), r, "ransac")
        return out[0:1].reshape(()).view(Homography)

    def hypotheses(self):
        """Every hypothesis record of the last fit as a HOMOGRAPHY_DTYPE array in index order (blocking)."""
        r = self._handle("ransac")
        _, most, _, _ = self.ransac_layout()
        out = np.zeros(most, HOMOGRAPHY_DTYPE)
        stored = ctypes.c_size_t()
        check(lib().gdp_download_hypotheses(r, _ptr(out), out.size, ctypes.byref(stored)), r, "ransac")
        return out[:stored.value]

    def inlier_count(self):
        """Inliers of the last fit (blocking; 0 before any and without a model)."""
        r = self._handles["ransac"]
        return _count("gdp_ransac_count", r, (), "ransac") if r.value else 0

    def inliers(self):
        """The last fit's inlier records as a MATCH_DTYPE array sorted by `query` (blocking); its
        `found` attribute is inlier_count()."""
        r = self._handles["ransac"]
        if not r.value:
            return np.zeros(0, MATCH_DTYPE).view(Keypoints)
        return _download("gdp_download_inliers", r, (), "ransac", MATCH_DTYPE, self.inlier_count())

    def device_inliers(self):
        """(device address of the inlier records, of their uint32 counter, of the model record)."""
        return _device_pointers("gdp_device_inliers", self._handle("ransac"), (), "ransac", n=3)

    def ransac_layout(self):
        """(capacity, max hypotheses, match chunk granule, hypotheses per block) of the fit object
        (gdp_ransac_layout)."""
        r = self._handle("ransac")
        cap = ctypes.c_size_t()
        most, mt, ht = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
        check(lib().gdp_ransac_layout(r, ctypes.byref(cap), ctypes.byref(most), ctypes.byref(mt), ctypes.byref(ht)), r, "ransac")
        return cap.value, most.value, mt.value, ht.value

    def refit_homography(self, rounds=1, threshold=3.0, stream=None):
        """Refit the last fit's model over its inliers by least squares on the device
        (gdp_refit_homography: exact 128-bit integer moments of the inlier coordinates quantised to
        1/256 px, one 8 x 8 solve in float64; a round's candidate replaces the model record and the
        inlier list in place when it accepts at least as many matches under `threshold`);
        asynchronous on `stream`, no host read, so warp_image and guided_match after it consume the
        refit model."""
        r = self._handle("ransac")
        check(lib().gdp_refit_homography(r, int(rounds), float(threshold), _stream_handle(stream)), r, "ransac")

    def refit_record(self):
        """The last refit's REFIT_DTYPE record (blocking; all 0 before any)."""
        r = self._handle("ransac")
        out = np.zeros(1, REFIT_DTYPE)
        check(lib().gdp_download_refit(r, _ptr(out)), r, "ransac")
        return out[0]

    # ------------------------------------------------------------------ guided matching (extension)
    # The gdp_guided object only reads the fit object and, through it, the match object's two sides.
    def set_guided_capacity(self, max_cells=0):
        """The most cells the grid of a guided match may have (0: 262,144).  Drops the earlier result
        and set_guided_model's matrix."""
        if int(max_cells) < 0:
            raise ValueError("a cell count must be >= 0")
        self._set_capacity("guided", (int(max_cells),))

    def guided_match(self, radius, ratio=0.0, max_distance=None, unique=True, query_image=0, train_image=0, stream=None):
        """Match the two lists of the last match again under the last fit's model record (or
        set_guided_model's matrix) on the device (gdp_match_guided: every query is projected into the
        train frame and compared with the train records within `radius` pixels of its projection in
        x and in y; exact nearest and second-nearest among those, ties to the lowest index; the ratio
        test (0: off) and the distance cap of match_descriptors; `unique` keeps one query per train
        record, the nearest, ties to the lowest query); asynchronous on `stream`, no host read of the
        model or of either counter."""
        g = self._handle("guided")
        cap = 0xffffffff if max_distance is None else int(max_distance)
        check(lib().gdp_match_guided(g, int(query_image), int(train_image), float(radius), float(ratio), cap, int(bool(unique)),
                                     _stream_handle(stream)), g, "guided")

    def set_guided_model(self, h):
        """Make the nine floats of `h` (3 x 3 or flat, row-major, query -> train) the model a guided
        match reads instead of the fit's model record (blocking; the floats are not validated); None
        goes back to the fit's record."""
        self._set_model("guided", h)

    def guided_count(self):
        """Records the last guided match produced (blocking; 0 before any)."""
        g = self._handles["guided"]
        return _count("gdp_guided_count", g, (), "guided") if g.value else 0

    def guided_matches(self):
        """The last guided match's records as a MATCH_DTYPE array sorted by `query` (blocking); its
        `found` attribute is guided_count()."""
        g = self._handles["guided"]
        if not g.value:
            return np.zeros(0, MATCH_DTYPE).view(Keypoints)
        return _download("gdp_download_guided", g, (), "guided", MATCH_DTYPE, self.guided_count())

    def device_guided(self):
        """(device address of the guided match records, device address of their uint32 counter)."""
        return _device_pointers("gdp_device_guided", self._handle("guided"), (), "guided")

    def guided_layout(self):
        """(cell side, cells per row, cells per column) of the last guided match's grid — 0, 0, 0
        before any — then (the most cells a grid may have, lanes per query) (gdp_guided_layout)."""
        g = self._handle("guided")
        side = ctypes.c_float()
        gx, gy, most, lanes = (ctypes.c_uint32() for _ in range(4))
        check(lib().gdp_guided_layout(g, ctypes.byref(side), ctypes.byref(gx), ctypes.byref(gy), ctypes.byref(most), ctypes.byref(lanes)),
              g, "guided")
        return side.value, gx.value, gy.value, most.value, lanes.value

    # ------------------------------------------------------------------ homography warp (extension)
    def warp_image(self, direction="train_to_query", query_image=0, train_image=0, fill=0, stream=None):
        """Resample one input image into the other's frame under the last fit's model record (or
        set_warp_model's matrix) on the device (gdp_warp_image: 'train_to_query' brings image
        `train_image` of the matched train context into image `query_image`'s frame of this context,
        'query_to_train' the other way round under the normalised adjugate; bilinear, ties to even,
        uncovered pixels store `fill`); asynchronous on `stream`, no host read of the model."""
        w = self._handle("warp")
        code = WARP_DIRECTIONS.get(direction, direction)
        check(lib().gdp_warp_image(w, int(code), int(query_image), int(train_image), int(fill), _stream_handle(stream)), w, "warp")

    def set_warp_model(self, h):
        """Make the nine floats of `h` (3 x 3 or flat, row-major, query -> train) the model a warp
        reads instead of the fit's model record (blocking; the floats are not validated); None goes
        back to the fit's."""
        self._set_model("warp", h)

    def warp_record(self):
        """The last warp's WARP_DTYPE record (blocking; all 0 before any)."""
        w = self._handle("warp")
        out = np.zeros(1, WARP_DTYPE)
        check(lib().gdp_download_warp_record(w, _ptr(out)), w, "warp")
        return out[0]

    def device_warped(self):
        """(device address of the warped image, pitch in elements, height, width, 'i32' or 'u8', device
        address of the record): what a context of that size and format binds with bind_device_input."""
        w = self._handle("warp")
        pix, rec, pitch = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_size_t()
        h, wd, fmt = _i(), _i(), _i()
        check(lib().gdp_device_warped(w, ctypes.byref(pix), ctypes.byref(pitch), ctypes.byref(h), ctypes.byref(wd), ctypes.byref(fmt),
                                      ctypes.byref(rec)), w, "warp")
        return pix.value, pitch.value, h.value, wd.value, "u8" if fmt.value == 1 else "i32", rec.value

    def warped(self):
        """The last warp's output as a numpy array of the destination frame's shape in the output
        format, int32 or uint8 (blocking; 0 x 0 before any)."""
        w = self._handle("warp")
        _, _, h, wd, fmt, _ = self.device_warped()
        out = np.zeros((h, wd), np.uint8 if fmt == "u8" else np.int32)
        if out.size:
            check(lib().gdp_download_warped(w, _ptr(out), wd), w, "warp")
        return out

    def warp_layout(self):
        """(rows, columns of a wave's tile of the destination frame, consecutive columns per lane)
        (gdp_warp_layout)."""
        w = self._handle("warp")
        tr, tc, ppl = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
        check(lib().gdp_warp_layout(w, ctypes.byref(tr), ctypes.byref(tc), ctypes.byref(ppl)), w, "warp")
        return tr.value, tc.value, ppl.value

    def device_level_ptr(self, b, o, s):
        """Device address of level (o, s) of image b.  Read-only: after writing through it, call
        pyramid_written() before the next build."""
        return lib().gdp_device_level(self._ctx, int(b), int(o), int(s))

    def pyramid_written(self, b=-1):
        """Image b's pyramid (b < 0: every image's) was written by something other than libgdp: the
        next build stores every byte again (gdp_pyramid_written)."""
        check(lib().gdp_pyramid_written(self._ctx, int(b)), self._ctx)

    def taps(self, axis, o, s):
        """Window the device holds: axis 0 = column taps (from W), 1 = row taps (from H)."""
        n = (self.W >> o) if axis == 0 else (self.H >> o)
        out = np.empty(n, np.float32)
        check(lib().gdp_get_taps(self._ctx, int(axis), int(o), int(s), _ptr(out)), self._ctx)
        return out

    # ------------------------------------------------------------------ lifetime
    def close(self):
        self._drop("orient")  # every stage object goes before its context
        if self._ctx.value:
            lib().gdp_destroy(self._ctx)
            self._ctx = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _TrackedBuffer:
    """gdp_host_alloc_tracked memory seen by numpy (GaussPyramid(defer=True)): arrays made from it
    keep it alive, and it is freed when the last one goes."""

    def __init__(self, nfloats):
        p = ctypes.c_void_p()
        check(lib().gdp_host_alloc_tracked(int(nfloats) * 4, ctypes.byref(p)))
        self.ptr = p.value
        self.__array_interface__ = {"shape": (int(nfloats),), "typestr": "<f4", "data": (self.ptr, False), "version": 3}

    def __del__(self):
        if getattr(self, "ptr", None):
            try:
                lib().gdp_host_free(ctypes.c_void_p(self.ptr))
            except Exception:  # interpreter shutdown: the process unmaps it anyway
                pass
            self.ptr = None


class _LevelView:
    """GaussPy[o] -> list of S+3 level arrays, downloaded on first access after a change."""

    def __init__(self, owner, o):
        self._owner, self._o = owner, o

    def __getitem__(self, s):
        return self._owner._level(self._o, s)

    def __setitem__(self, s, value):  # GaussPy[o][s] = array: the level's new contents
        self._owner._level(self._o, s)[...] = value

    def __len__(self):
        return self._owner.S + 3


class GaussPyramid:
    """GPU mirror of `class GaussPyramid` (GuassDePyramid.h:11-29); see the module docstring."""

    def __init__(self, img=None, len=None, S=2, device=0, defer=False):  # noqa: A002  (reference argument name)
        # GaussPyramid() (GuassDePyramid.h:31-34): empty object
        self.data = None
        self.initialized = False
        self._defer = False
        self._ctx = None
        if img is None:
            return
        length = int(len)
        # :38-46 deep copy of img[0:len][0:len] (img may be larger, as in main.cpp:27-35,61)
        self.data = np.array([np.asarray(img[i][:length], dtype=np.int32) for i in range(length)], dtype=np.int32)
        self.length = length
        self.S = int(S)
        self.layer = octaves_for(length)  # :48-53
        self._ctx = PyramidContext(length, length, self.S, self.layer, batch=1, device=device)
        self._cache = {}  # (o, s) -> the level's host array (live for the object's lifetime)
        self._snap = {}  # (o, s) -> the bits the device last gave that array (edit detection)
        self._raw = None  # one host buffer in the device's raw image layout; the levels are views
        self._fresh = False
        self.uploaded_levels = 0  # levels the last SyncDevice uploaded (0: the host held no edits)
        if defer:
            # deferred download (round 6, the C++ classes' DeferDownload): the levels are views of a
            # write-tracked mirror (gdp_host_alloc_tracked) whose pages are fetched from the device
            # when first touched after a call; edits are found by page faults, not by comparison
            self._raw = np.asarray(_TrackedBuffer(lib().gdp_image_floats(self._ctx._ctx)))
            self._defer = True
            self.uploaded_bytes = 0
        self.GaussPyInit()  # :57

    # reference surface -------------------------------------------------------
    def GaussPyInit(self):
        """:60-87 — refill every level of every octave with the decimated CURRENT `data` (:80)."""
        self._ctx.set_input(self.data)
        self._ctx.init()
        self.initialized = True
        self._fresh = True  # contents == init, so GenerateDoG may take the fused path
        self._refresh()  # every level refilled: host edits are overwritten, as in :76-86

    def GaussFilter(self, theLayer):
        """:106-134 — multiply every scale of octave `theLayer` by its window, in place."""
        self.SyncDevice()
        self._ctx.gauss_octave(int(theLayer))
        self._fresh = False
        self._refresh()

    def GenerateDoG(self):
        """:136-149 — GaussFilter + DoG for every octave, in place on the current contents."""
        self.SyncDevice()
        if self._fresh:
            self._ctx.build()  # fused init+filter+DoG: bit-identical to the in-place sequence
        else:
            self._ctx.generate_dog()
        self._fresh = False
        self._refresh()

    def DetectExtrema(self, contrast=0.0, edge_ratio=0.0):
        """Extension (no reference counterpart): the strict scale-space extrema of the current
        pyramid, found on the device (PyramidContext.detect_extrema), as a KEYPOINT_DTYPE array
        sorted by (octave, scale, row, col).  Host edits to GaussPy are detected on; the pyramid is
        not changed, so nothing is refreshed or downloaded but the records."""
        self.SyncDevice()
        self._ctx.detect_extrema(contrast, edge_ratio)
        return self._ctx.keypoints(0)

    def RefineKeypoints(self, contrast=0.0, edge_ratio=0.0):
        """Extension: refine the last DetectExtrema's keypoints to sub-sample precision on the
        device (PyramidContext.refine_keypoints) and return them as a REFINED_DTYPE array.  Host
        edits to GaussPy are refined on; the pyramid is not changed."""
        self.SyncDevice()
        self._ctx.refine_keypoints(contrast, edge_ratio)
        return self._ctx.refined_keypoints(0)

    def OrientKeypoints(self):
        """Extension: assign orientations to the last RefineKeypoints' records on the device
        (PyramidContext.orient_keypoints) and return one ORIENTED_DTYPE record per histogram peak.
        Host edits to GaussPy are oriented on; the pyramid is not changed."""
        self.SyncDevice()
        self._ctx.orient_keypoints()
        return self._ctx.oriented_keypoints(0)

    def DescribeKeypoints(self):
        """Extension: compute the SIFT descriptors of the last OrientKeypoints' records on the device
        (PyramidContext.describe_keypoints) and return one DESCRIBED_DTYPE record per oriented
        keypoint.  Host edits to GaussPy are described on; the pyramid is not changed."""
        self.SyncDevice()
        self._ctx.describe_keypoints()
        return self._ctx.described_keypoints(0)

    def MatchDescriptors(self, other=None, ratio=0.8, max_distance=None, mutual=False):
        """Extension: match the last DescribeKeypoints' records of this pyramid (the queries) against
        those of `other` (another GaussPyramid on the same device; None: this one) on the device
        (PyramidContext.match_descriptors) and return the MATCH_DTYPE records sorted by `query`.
        Neither pyramid nor any list is changed."""
        self._ctx.match_descriptors(None if other is None else other._ctx, 0, 0, ratio, max_distance, mutual)
        return self._ctx.matches()

    def FitHomography(self, matches=None, hypotheses=1024, seed=0, threshold=3.0, min_inliers=4):
        """Extension: fit a homography to `matches` (MATCH_DTYPE records in the order given; None:
        the last MatchDescriptors' list where it lies on the device, in device order) by RANSAC on
        the device (PyramidContext.fit_homography) and return (the model record, whose `matrix` is
        the 3 x 3 array or None, the inlier records sorted by `query`).  Nothing else is changed."""
        self._ctx.set_ransac_input(matches)
        self._ctx.fit_homography(hypotheses, seed, threshold, min_inliers)
        return self._ctx.homography(), self._ctx.inliers()

    def RefitHomography(self, rounds=1, threshold=3.0):
        """Extension: refit the last FitHomography's model over its inliers by least squares on the
        device (PyramidContext.refit_homography) and return (the model record, the inlier records
        sorted by `query`, the REFIT_DTYPE record).  Nothing else is changed."""
        self._ctx.refit_homography(rounds, threshold)
        return self._ctx.homography(), self._ctx.inliers(), self._ctx.refit_record()

    def WarpImage(self, other=None, model=None, direction="train_to_query", fill=0):
        """Extension: resample `other`'s input image (the train side; None: the train side of the
        last MatchDescriptors, or this pyramid) into this pyramid's frame — or, with
        direction='query_to_train', this pyramid's into `other`'s — under `model` (nine floats mapping
        this pyramid's (x, y) to `other`'s; None: the last FitHomography's model record, read on the
        device) on the device (PyramidContext.warp_image).  Returns (the warped image, int32, and the
        WARP_DTYPE record with `covered` and `sad`).  Neither pyramid nor any list is changed."""
        if other is not None:
            self._ctx._handle("match", other._ctx)
        self._ctx.set_warp_model(model)
        self._ctx.warp_image(direction, 0, 0, fill)
        return self._ctx.warped(), self._ctx.warp_record()

    def GuidedMatch(self, other=None, model=None, radius=3.0, ratio=0.0, max_distance=None, unique=True):
        """Extension: match the last DescribeKeypoints' records of this pyramid against those of
        `other` (None: the train side of the last MatchDescriptors, or this pyramid) again, each
        query only against the records within `radius` pixels of its projection under `model` (nine
        floats mapping this pyramid's (x, y) to `other`'s; None: the last FitHomography's model
        record, read on the device) on the device (PyramidContext.guided_match).  Returns the
        MATCH_DTYPE records sorted by `query`.  Neither pyramid nor any list is changed."""
        if other is not None:
            self._ctx._handle("match", other._ctx)
        self._ctx.set_guided_model(model)
        self._ctx.guided_match(radius, ratio, max_distance, unique)
        return self._ctx.guided_matches()

    def output(self, file=None):
        """:89-104 — print scale 0 of each octave (space separated) and an `==` separator row."""
        file = sys.stdout if file is None else file
        n = self.length
        for o in range(self.layer):
            lev = self._level(o, 0)
            for row in lev:
                file.write("".join(f"{v:g} " for v in row) + "\n")
            file.write("==" * n + "\n")
            n //= 2

    @property
    def GaussPy(self):
        return [_LevelView(self, o) for o in range(self.layer)]

    def SyncDevice(self):
        """Upload every level the caller obtained through GaussPy AND changed (its bits differ from
        the device's last copy) into the device pyramid; the next call processes the host contents.
        Sets `uploaded_levels`.  With defer=True: the pages written since the last call
        (`uploaded_bytes`; `uploaded_levels` is 0 when nothing was written, else -1)."""
        if self._defer:
            w = ctypes.c_size_t()
            written = w.value if lib().gdp_host_written_bytes(_ptr(self._raw), ctypes.byref(w)) == 0 else None
            check(lib().gdp_upload_image_written(self._ctx._ctx, 0, _ptr(self._raw)), self._ctx._ctx)
            self.uploaded_bytes = written
            self.uploaded_levels = 0 if written == 0 else -1
            if written != 0:
                self._fresh = False
            return
        n = 0
        for key, arr in self._cache.items():
            snap = self._snap[key]
            if not np.array_equal(arr.view(np.uint32), snap.view(np.uint32)):
                self._ctx.upload_level(0, key[0], key[1], arr)
                snap[...] = arr
                n += 1
        self.uploaded_levels = n
        if n:
            self._fresh = False  # the caller's contents, not necessarily GaussPyInit's

    # helpers -----------------------------------------------------------------
    def _level(self, o, s):
        key = (o, s)
        if key not in self._cache and self._defer:  # a view of the deferred mirror: fetched on touch
            rows, cols = self._ctx.level_dims(o)[:2]
            off = self._ctx.level_offset(0, o, s)
            self._cache[key] = self._raw[off:off + rows * cols].reshape(rows, cols)
        if key not in self._cache:
            if self._raw is None:
                self._raw = np.empty(lib().gdp_image_floats(self._ctx._ctx), np.float32)
            rows, cols = self._ctx.level_dims(o)[:2]
            off = self._ctx.level_offset(0, o, s)
            arr = self._raw[off:off + rows * cols].reshape(rows, cols)
            self._ctx.sync()
            if arr.size:
                check(lib().gdp_download_level(self._ctx._ctx, 0, int(o), int(s), _ptr(arr)), self._ctx._ctx)
            self._cache[key] = arr
            self._snap[key] = arr.copy()
        return self._cache[key]

    def _refresh(self):
        """After a device-side change: every touched level re-downloaded INTO its existing array,
        so handles the caller holds stay live (the reference's rows never move) — in one raw copy
        of the image when the touched levels are at least half of its bytes, else level by level.
        With defer=True: nothing is copied — the mirror is deferred (gdp_host_defer)."""
        if self._defer:
            self._ctx.sync()
            check(lib().gdp_host_defer(self._ctx._ctx, 0, _ptr(self._raw)), self._ctx._ctx)
            return
        if not self._cache:
            return
        self._ctx.sync()
        touched = sum(arr.size for arr in self._cache.values())
        if 2 * touched >= self._raw.size:
            check(lib().gdp_download_image_raw(self._ctx._ctx, 0, _ptr(self._raw)), self._ctx._ctx)
        else:
            for (o, s), arr in self._cache.items():
                if arr.size:
                    check(lib().gdp_download_level(self._ctx._ctx, 0, int(o), int(s), _ptr(arr)), self._ctx._ctx)
        for key, arr in self._cache.items():
            self._snap[key][...] = arr

    def pyramid(self):
        """Packed [o][s][r][c] float32 copy (the oracle's layout)."""
        return self._ctx.pyramid(0)

    def close(self):
        if self._ctx is not None:
            self._ctx.close()


class GaussPyramid_a512omp(GaussPyramid):
    """GPU mirror of `class GaussPyramid_a512omp` (GaussDePyramid-AVX512xOpenMP.h:20-48), the
    reference's timed AVX-512 x OpenMP path; same object model as GaussPyramid (include/
    GaussDePyramid-HIP-AVX512.h is the C++ form).  Window centre: that header's integer length."""

    counnt = 2  # GaussDePyramid-AVX512xOpenMP.h:18 (a global there; no effect on the GPU)

    def __init__(self, img=None, len=None, S=2, device=0, defer=False):  # noqa: A002
        super().__init__(img, len, S, device, defer)
        if img is not None:
            self._ctx.set_window_centre("intlen")

    def GaussFilter(self, theLayer):
        """:128-181 — the reference's body is commented out: nothing happens."""

    def GenerateDoG(self):
        """:183-213 — DoG pass only (level j -= level j+1, j = 0..S+1) per octave, twice on octaves
        of side <= 2."""
        self.SyncDevice()
        self._ctx.dog_range(0, self.layer)  # one launch for every octave ...
        tiny = next((o for o in range(self.layer) if self.length >> o <= 2), self.layer)
        if tiny < self.layer:
            self._ctx.dog_range(tiny, self.layer)  # ... and one for the repeat on sides <= 2
        self._fresh = False
        self._refresh()

    def GenerateDoG_nomp_dynamic(self):
        """:240-364 — scales 0..S-1 windowed, DoG for i < S-1: {DoG_0..DoG_{S-2}, G_{S-1}, x, x, x}."""
        self.SyncDevice()
        if self._fresh:
            self._ctx.build_subset()
        else:
            self._ctx.generate_dog_subset()
        self._fresh = False
        self._refresh()

    def GenerateDoG_nomp_static(self):
        """:366-368 — empty in the reference."""


class GaussPyramid_a512xp(GaussPyramid):
    """GPU mirror of `class GaussPyramid_a512xp` (GaussDePyramid-AVX512xPTHREAD.h:21-40): full
    semantics; GenerateDoG with that header's integer-length centre (:193, :218), GaussFilter with
    the serial float-halved one (:113-141)."""

    def __init__(self, img=None, len=None, S=2, device=0, defer=False):  # noqa: A002
        super().__init__(img, len, S, device, defer)
        if img is not None:
            self._ctx.set_window_centre("intlen")

    def GaussFilter(self, theLayer):
        self._ctx.set_window_centre("serial")
        try:
            super().GaussFilter(theLayer)
        finally:
            self._ctx.set_window_centre("intlen")
