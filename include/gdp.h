/*
 * gdp.h — C ABI of libgdp.so, the MI355X (gfx950) Gaussian / Difference-of-Gaussians pyramid.
 *
 * This is the drop-in boundary for the reference's pyramid hot path
 * (ZhangShuui/SIFT-parallel-optimization, GuassDePyramid.h and the GaussDePyramid-*.h variants).
 * The reference exposes a duck-typed C++ class surface selected by #include (main.cpp:2-13);
 * every entry point below names the reference member it replaces (file:line).  The C++ class
 * `GaussPyramid_hip` (include/GaussDePyramid-HIP.h) and the Python mirror
 * (sift-parallel-optimization_amd/gausspyramid.py) are thin callers of exactly these functions.
 *
 * Conventions
 *  - Every function returns an int status (GDP_OK == 0) unless documented otherwise; no C++
 *    exception crosses the ABI.  gdp_last_error(ctx) / gdp_status_string() describe failures.
 *  - Only plain pointers and sizes cross the boundary.  `stream` is a hipStream_t passed as
 *    void*: NULL = the context's own stream, GDP_STREAM_NULL = HIP's default (null) stream; all
 *    compute and copy calls are stream-ordered and asynchronous unless documented otherwise.
 *  - The context owns its device buffers (input, pyramid, tap tables); the caller keeps
 *    ownership of every host array it passes in.  One context per host thread and device.
 *  - Semantics are the reference's, bit for bit: float32 taps from glibc expf/sqrtf computed on
 *    the host (GuassDePyramid.h:119-121), products ((float)x * f[c]) * f[r] with no FMA
 *    contraction and denormals kept, DoG_s = G_s - G_{s+1} in ascending s (:140-146),
 *    level S+2 keeps the last Gaussian.
 *
 * Pyramid geometry (per image b of a batch):
 *   octave o has rows_o x cols_o pixels, cols_o = W >> o and (whole image) rows_o = H >> o;
 *   scale s in [0, S+3).  Octave o decimates the ORIGINAL image: input pixel (r<<o, c<<o)
 *   (GuassDePyramid.h:80).  `octaves` = 0 selects floor(log2(min(H, W))) + 1, the reference's
 *   `layer` (GuassDePyramid.h:48-53).  The reference is square-only; H != W is an extension
 *   (W-derived window along columns, H-derived window along rows).
 *   A "band" context computes the output rows whose input rows lie in [row_begin, row_end) of
 *   an H-row image (multi-GPU row-band partition; the operation is pointwise, halo = 0).
 */
#ifndef GDP_H_
#define GDP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gdp_ctx gdp_ctx;

/* Stream argument selecting HIP's default (null) stream; NULL selects the context's stream. */
#define GDP_STREAM_NULL ((void*)1)

enum {
    GDP_OK = 0,
    GDP_ERR_ARG = 1,      /* invalid argument (sizes, indices, null pointers)        */
    GDP_ERR_HIP = 2,      /* a HIP runtime call failed (message in gdp_last_error)   */
    GDP_ERR_STATE = 3,    /* call not valid in the context's current state           */
    GDP_ERR_NOMEM = 4,    /* host or device allocation failed                        */
    GDP_ERR_NODEV = 5,    /* no usable gfx950 device                                 */
    GDP_ERR_INTERNAL = 6  /* unexpected internal failure (a C++ exception stopped at the ABI) */
};

/* ABI version of this header; gdp_abi_version() returns the library's. */
#define GDP_ABI_VERSION 1
int gdp_abi_version(void);

/* Number of visible HIP devices (0 when none / no driver). */
int gdp_device_count(void);

/* Number of octaves the reference builds for an n-pixel axis: floor(log2 n) + 1
 * (GaussPyramid ctor, GuassDePyramid.h:48-53). */
int gdp_octaves_for(int n);

/* Allocate a context for `batch` images of H x W int32 pixels, S (+3 Gaussian scales per octave)
 * and `octaves` octaves (0 = all) on HIP device `device`, and upload the tap tables.
 * Replaces the allocation half of GaussPyramid(int** img, int len, int S)
 * (GuassDePyramid.h:36-58) and GaussPyInit's first-call allocation (:60-73). */
int gdp_create(gdp_ctx** out, int height, int width, int S, int octaves, int batch, int device);

/* Same as gdp_create for the row band [row_begin, row_end) of an H-row image.  row_begin must
 * be a multiple of 2^(max(octaves,5)-1); row_end must be too, or equal `height`.  Extension for
 * the multi-GPU row-band split (no reference counterpart). */
int gdp_create_band(gdp_ctx** out, int height, int width, int S, int octaves, int batch, int row_begin,
                    int row_end, int device);

/* Free every device buffer.  Replaces ~GaussPyramid() (GuassDePyramid.h:151-170). */
void gdp_destroy(gdp_ctx* ctx);

/* Geometry queries.  gdp_level_dims gives the rows held by this context for octave o (the whole
 * image, or the band), their first global row, and the columns. */
int gdp_get_geometry(const gdp_ctx* ctx, int* height, int* width, int* S, int* octaves, int* batch);
int gdp_level_dims(const gdp_ctx* ctx, int octave, int* rows, int* cols, int* first_row);
size_t gdp_pyramid_bytes(const gdp_ctx* ctx); /* device bytes of all pyramids of the batch */
/* The pyramid's backing: by default one reserved address range backed by separately
 * created 2 MiB physical pieces (GDP_TUNE_PYRAMID_CHUNK_KB reports it); GDP_SPREAD_VMM=0 in the
 * environment when the context is created gives one hipMalloc instead (e.g. to share the pyramid
 * with another process through IPC).  Identical bits and offsets either way.  Each image starts
 * on an allocation granule only where that wastes at most 1/16 of an image: gdp_pyramid_bytes and
 * gdp_level_offset follow that stride, gdp_image_floats stays one image's dense extent.  (The
 * layout experiments of DESIGN.md §4 read further variables only in the research build,
 * `make -C sift-parallel-optimization_amd/csrc exp`.) */

/* ---- input ---------------------------------------------------------------------------------
 * The reference deep-copies `int** img` in its constructor (GuassDePyramid.h:38-46).  These
 * upload image b of the batch (band contexts: the band's rows only, given as rows of the band). */
/* int** row-pointer form, exactly the reference ctor's argument. */
int gdp_set_input_rows(gdp_ctx* ctx, int b, const int32_t* const* rows, void* stream);
/* contiguous host image with a row pitch of `pitch` int32 elements. */
int gdp_set_input_host(gdp_ctx* ctx, int b, const int32_t* base, size_t pitch, void* stream);
/* Zero-copy: read every image straight from caller-owned DEVICE memory.  Image b, row r starts
 * at base + b*image_stride + r*pitch (int32 elements).  Pass base = NULL to go back to the
 * context's own input buffer.  The memory must stay valid while builds run. */
int gdp_set_input_device(gdp_ctx* ctx, const int32_t* base, size_t pitch, size_t image_stride);
/* Input pixel format of the context: GDP_INPUT_I32 (default; the reference's int) or
 * GDP_INPUT_U8 (8-bit images: a quarter of the input bytes, identical pyramid bits since every
 * uint8 value is an int).  Switching reallocates the context's input buffer (contents zeroed). */
enum { GDP_INPUT_I32 = 0, GDP_INPUT_U8 = 1 };
int gdp_set_input_format(gdp_ctx* ctx, int format);
int gdp_get_input_format(const gdp_ctx* ctx);
int gdp_set_input_host_u8(gdp_ctx* ctx, int b, const uint8_t* base, size_t pitch, void* stream);
int gdp_set_input_device_u8(gdp_ctx* ctx, const uint8_t* base, size_t pitch, size_t image_stride);
/* Benchmark/test input generated on the device (SURVEY.md §8d counter hash): image b of the
 * batch gets global index first_image + b; pixel = lowbias32(seed ^ fold(idx)) >> 24 with
 * idx = (index*H + r)*W + c over the WHOLE image (band contexts generate their rows only).
 * Writes the input the builds read: the context's own buffer, or the caller's device buffer
 * bound by gdp_set_input_device* (its pitch and image stride; the pitch padding is untouched). */
int gdp_fill_synthetic(gdp_ctx* ctx, uint32_t seed, long first_image, void* stream);

/* ---- compute ------------------------------------------------------------------------------- */
/* Fused GaussPyInit() + GenerateDoG() for every image of the batch in one launch: reads each
 * input pixel once and writes the final pyramid once.  Equivalent, bit for bit, to
 * GuassDePyramid.h:74-86 followed by :136-149. */
int gdp_build(gdp_ctx* ctx, void* stream);
/* GaussPyInit() refill: every scale of octave o := (float) decimated input
 * (GuassDePyramid.h:74-86). */
int gdp_init(gdp_ctx* ctx, void* stream);
/* GaussFilter(o) in place: every scale of octave o *= column window then row window
 * (GuassDePyramid.h:106-134). */
int gdp_gauss_octave(gdp_ctx* ctx, int octave, void* stream);
/* GaussFilter(o) for every o in [o_begin, o_end) in ONE launch (the reference calls it per octave
 * from GenerateDoG, :139); the "row + column window pass" the north star's roofline target names. */
int gdp_gauss_range(gdp_ctx* ctx, int o_begin, int o_end, void* stream);
/* The window multiply of scales [s_begin, s_end) only, for every octave in [o_begin, o_end), in
 * ONE launch: what worker rank i of the reference's MPI variant does to its own scale i before
 * sending it to the collector (GaussPyramid_mpi::GenerateDoG_mpi, GaussDePyramid-MPI.h:271-290;
 * its integer-length centre is GDP_CENTRE_INTLEN).  gdp_gauss_range is s = [0, S+3). */
int gdp_gauss_scales(gdp_ctx* ctx, int s_begin, int s_end, int o_begin, int o_end, void* stream);
/* DoG of octave o in place: level s -= level s+1 for s = 0..S+1 ascending
 * (GuassDePyramid.h:140-146). */
int gdp_dog_octave(gdp_ctx* ctx, int octave, void* stream);
/* The DoG pass of every octave in [o_begin, o_end) in ONE launch (no window multiply). */
int gdp_dog_range(gdp_ctx* ctx, int o_begin, int o_end, void* stream);
/* GenerateDoG() in place on the CURRENT contents, all octaves in one launch
 * (GuassDePyramid.h:136-149).  After gdp_init this equals gdp_build; called again it re-filters,
 * like the reference's repeated-call timing loop (main.cpp:66-73). */
int gdp_generate_dog(gdp_ctx* ctx, void* stream);
/* GaussPyramid_a512omp::GenerateDoG_nomp_dynamic (GaussDePyramid-AVX512xOpenMP.h:240-364), the
 * reference's AVX-512 x OpenMP path, whose output is a SUBSET of GenerateDoG's: only scales
 * 0..S-1 are windowed (:242-318) and level i -= level i+1 only for i < S-1 (:337-357), so the
 * pyramid holds {DoG_0..DoG_{S-2}, G_{S-1}, x, x, x} with x the GaussPyInit value.  The header
 * computes its windows with the integer-length centre float(len_o - 1) / 2 (:251, :279): use
 * GDP_CENTRE_INTLEN (gdp_set_window_centre) to reproduce it (identical to the serial centre when
 * the side is a multiple of 2^(octaves-1), the only sizes its 16-float vector loops handle).
 *   gdp_build_subset:        fused GaussPyInit + GenerateDoG_nomp_dynamic from the input
 *   gdp_generate_dog_subset: GenerateDoG_nomp_dynamic in place on the CURRENT contents (repeated
 *                            calls re-filter, like the reference's timing loop) */
int gdp_build_subset(gdp_ctx* ctx, void* stream);
int gdp_generate_dog_subset(gdp_ctx* ctx, void* stream);

/* ---- extension: true Gaussian convolution pyramid --------------------------
 * NOT the reference's algorithm (which multiplies by a window, :119-131) and carries no parity
 * claim: G_s = base_o (*) k_s, the separable Gaussian with sigma_s = 2/(s+1) (the reference's
 * schedule), normalised taps over radius ceil(3 sigma_s) (<= 6), clamp-to-edge borders; same octave
 * bases, DoG and level layout as gdp_build.  Row bands need their halo rows (below).
 * gdp_conv_taps returns scale s's 13 taps (zero beyond 2R+1) and radius R. */
int gdp_build_gaussian(gdp_ctx* ctx, void* stream);
int gdp_conv_taps(int S, int scale, float* taps13, int* radius);
/* Row bands (multi-GPU split of one image): unlike the reference's
 * pointwise window, the convolution reads 6 rows of every octave beyond a band's own rows, i.e.
 * up to 6 * 2^(octaves-1) input rows above and below it (clipped to the image): *above / *below
 * (0 for whole-image contexts).  A band's gdp_build_gaussian reads them from halo buffers
 * [batch][rows][pitch] (the context's input format): the context's own (gdp_input_halo allocates
 * one on first call, binds it and returns its device address — later calls only return it, with
 * no geometry upload — for a neighbour's rows to be written into —
 * gdp_comm_exchange_halo over RCCL, or any copy) or caller device memory (gdp_bind_input_halo,
 * zero copy; pitch and image stride multiples of 4, rows 16-B aligned).  gdp_device_input returns
 * the device address and pitch of image b's input rows (the context's own or a bound buffer), the
 * rows a neighbour needs.  A band build fails with GDP_ERR_STATE until both halos it needs are
 * set, and only the block-tile kernel (GDP_TUNE_CONV_KERNEL 2, S <= 5, width a multiple of
 * 2^(octaves+1)) runs on bands; its output equals the whole image's rows bit for bit. */
int gdp_conv_halo_rows(const gdp_ctx* ctx, int* above, int* below);
int gdp_input_halo(gdp_ctx* ctx, int side /* 0 above, 1 below */, void** rows, size_t* pitch);
int gdp_bind_input_halo(gdp_ctx* ctx, const void* above, const void* below, size_t pitch, size_t image_stride);
int gdp_device_input(const gdp_ctx* ctx, int b, const void** rows, size_t* pitch);

/* ---- extension: scale-space extrema (keypoints) on the device ---------------------------------
 * The next SIFT step done where the pyramid already is (no reference counterpart, no parity claim):
 * the local extrema of the DoG levels in space and scale, as a compact list of 16-byte records —
 * a caller needs no host copy of the pyramid to find them.  It runs on whatever the pyramid
 * CURRENTLY holds (the context's own buffer or one bound with gdp_set_output_device): most
 * meaningful after gdp_build_gaussian, whose DoG is a real scale space, but the reference's window
 * pyramid works too.  gdp_refine_keypoints (below) localises them to sub-sample precision and
 * gdp_orient_keypoints (below it) assigns their orientations.  Out of scope: descriptors.
 * (That was the scope of this step alone: gdp_describe_keypoints, further below, now provides them.)
 *
 * For image b and octave o (rows x cols as held by the context), levels 0..S+1 are taken as the
 * DoG levels D; level S+2 is never read.  Candidates are s in [1, S], r in [1, rows-2],
 * c in [1, cols-2]; octaves under 3 x 3 and contexts with S = 0 yield nothing (the calls succeed,
 * count 0).  A candidate v = D[s][r][c] is a keypoint when
 *   1. it is a STRICT extremum: v > n for all 26 neighbours n in {s-1,s,s+1} x {r-1,r,r+1} x
 *      {c-1,c,c+1} (kind +1), or v < n for all 26 (kind -1).  Plain IEEE float32 comparisons,
 *      denormals kept: ties are not extrema (the window pyramid's +0 plateaus give nothing),
 *      -0 == +0, and a NaN among the 27 values disqualifies the candidate;
 *   2. fabsf(v) > contrast_threshold;
 *   3. when edge_ratio != 0, with every operation a separately rounded float32 operation (no
 *      contraction) in exactly this order
 *        dxx = (D[s][r][c+1] + D[s][r][c-1]) - 2.0f*v
 *        dyy = (D[s][r+1][c] + D[s][r-1][c]) - 2.0f*v
 *        dxy = ((D[s][r+1][c+1] - D[s][r+1][c-1]) - (D[s][r-1][c+1] - D[s][r-1][c-1])) * 0.25f
 *        tr  = dxx + dyy,  det = dxx*dyy - dxy*dxy
 *      det > 0.0f && (tr*tr)*edge_ratio < ((edge_ratio+1.0f)*(edge_ratio+1.0f))*det.
 * The result is an exact set.  contrast_threshold must be >= 0 (not NaN), edge_ratio 0 or finite
 * and >= 1 (GDP_ERR_ARG otherwise).  Row-band contexts are refused with GDP_ERR_STATE (the
 * neighbourhood crosses band edges); whole-image contexts of any batch size are supported;
 * contexts with S x (pixels of one image's octaves) >= 2^32 are refused with GDP_ERR_ARG (the
 * counter is 32-bit). */
typedef struct gdp_keypoint {   /* 16 bytes, one 16-B store per record */
    uint16_t octave; uint8_t scale; int8_t kind;   /* +1 maximum, -1 minimum */
    int32_t row, col;                               /* in level (octave, scale) */
    float value;                                    /* D[scale][row][col] */
} gdp_keypoint;
/* Records the context keeps per image (default 65536).  The context owns a [batch][capacity]
 * record buffer and [batch] uint32 counters, allocated on first use; setting another capacity
 * reallocates the buffer (after draining the device; earlier results are dropped).  0 is
 * GDP_ERR_ARG. */
int gdp_set_keypoint_capacity(gdp_ctx* ctx, size_t per_image);
/* Detect on every image of the batch: zeroes the counters on `stream`, then ONE launch over all
 * images and octaves (asynchronous and stream-ordered, like gdp_build).  More keypoints may be
 * found than the capacity holds: the counter still counts them all, the buffer then holds exactly
 * `capacity` distinct true keypoints (which ones is unspecified) and nothing is stored at or
 * beyond `capacity`.  The device order of the records is unspecified. */
int gdp_detect_extrema(gdp_ctx* ctx, float contrast_threshold, float edge_ratio, void* stream);
/* Keypoints the last detection found in image b (blocking; waits for the context's OWN stream,
 * like the blocking copies below; 0 before any detection). */
int gdp_keypoint_count(gdp_ctx* ctx, int b, size_t* found);
/* Copy min(found, the context's capacity, `capacity`) records of image b to `host` (blocking),
 * sorted ascending by (octave, scale, row, col), so host results are the same run to run.
 * *stored = records written, *found = gdp_keypoint_count (either may be NULL). */
int gdp_download_keypoints(gdp_ctx* ctx, int b, gdp_keypoint* host, size_t capacity,
                           size_t* stored, size_t* found);
/* Zero-copy view for device consumers: image b's record buffer (capacity records, the first
 * min(*count, capacity) valid, device order) and its counter.  GDP_ERR_STATE before the buffer
 * exists (first gdp_detect_extrema or gdp_set_keypoint_capacity). */
int gdp_device_keypoints(const gdp_ctx* ctx, int b, const gdp_keypoint** records, const uint32_t** count);

/* ---- extension: sub-pixel keypoint refinement on the device -----------------------------------
 * Lowe's localisation step, done where the pyramid and the keypoint list already are (no reference
 * counterpart, no parity claim): a 3-D quadratic is fitted to the DoG around every record of the
 * context's keypoint list, the sample moves to its neighbour while the fitted extremum lies more
 * than half a sample away, and low-contrast and edge-like points are rejected at the interpolated
 * position.  It reads levels 0..S+1 of the CURRENT pyramid (own or bound); level S+2 is never read.
 *
 * The rule.  Every operation is a separately rounded float32 operation: no contraction, denormals
 * kept, `/` is IEEE-correct division.  For a record (o, s, r, c), with D the levels of octave o
 * (rows x cols), repeat at most GDP_REFINE_MAX_STEPS times:
 *   v   = D[s][r][c]
 *   gc  = (D[s][r][c+1] - D[s][r][c-1]) * 0.5f      gr, gs likewise along r and s
 *   hcc = (D[s][r][c+1] + D[s][r][c-1]) - 2.0f*v    hrr, hss likewise
 *   hrc = ((D[s][r+1][c+1] - D[s][r+1][c-1]) - (D[s][r-1][c+1] - D[s][r-1][c-1])) * 0.25f
 *   hsc = ((D[s+1][r][c+1] - D[s+1][r][c-1]) - (D[s-1][r][c+1] - D[s-1][r][c-1])) * 0.25f
 *   hsr = ((D[s+1][r+1][c] - D[s+1][r-1][c]) - (D[s-1][r+1][c] - D[s-1][r-1][c])) * 0.25f
 *   A = hrr*hss - hsr*hsr   B = hrc*hss - hsc*hsr   C = hrc*hsr - hsc*hrr
 *   E = hcc*hss - hsc*hsc   Q = hcc*hsr - hrc*hsc   G = hcc*hrr - hrc*hrc
 *   det = (hcc*A - hrc*B) + hsc*C
 *   reject unless fabsf(det) > 0.0f                       (zero or NaN)
 *   xc = -(((A*gc - B*gr) + C*gs) / det)
 *   xr = -(((E*gr - B*gc) - Q*gs) / det)
 *   xs = -(((C*gc - Q*gr) + G*gs) / det)
 *   if fabsf(xc) <= 0.5f && fabsf(xr) <= 0.5f && fabsf(xs) <= 0.5f:  converged, stop
 *   c += (xc > 0.5f) - (xc < -0.5f); same for r with xr and s with xs   (one sample per axis and step)
 *   reject if nothing moved (a NaN offset), or if now s<1 || s>S || r<1 || r>rows-2 || c<1 || c>cols-2
 * A record that has not converged after GDP_REFINE_MAX_STEPS solves is rejected.  At convergence
 *   interp = v + ((gc*xc + gr*xr) + gs*xs) * 0.5f
 * and the record is kept when fabsf(interp) > contrast_threshold (a NaN fails) and, when
 * edge_ratio != 0, it also passes the edge test of gdp_detect_extrema (3. above) with dxx = hcc,
 * dyy = hrr, dxy = hrc taken at the final sample.  The kept record holds the final (s, r, c), v,
 * (xs, xr, xc), interp and the input's kind.  Two inputs that end at the same sample both stay, as
 * identical records: the result is an exact multiset.  A consumer's image coordinates are
 * (col + dcol) * 2^octave and (row + drow) * 2^octave. */
typedef struct gdp_keypoint_refined {   /* 32 bytes */
    uint16_t octave; uint8_t scale; int8_t kind;  /* kind copied from the input record */
    int32_t row, col;                             /* the FINAL sample (after moves) */
    float value;                                  /* D[scale][row][col] at the final sample */
    float dscale, drow, dcol;                     /* offset from the final sample, each |.| <= 0.5 */
    float interp;                                 /* interpolated DoG value at the offset */
} gdp_keypoint_refined;   /* its first 16 bytes are a gdp_keypoint at the final sample */
#define GDP_REFINE_MAX_STEPS 5
/* Refine every image's keypoint list: the first min(counter, keypoint capacity) records, read on
 * the device — the host never reads the counter, so launching this right after gdp_detect_extrema
 * on the same stream is the normal use (the caller orders the two when the streams differ).
 * Asynchronous and stream-ordered: zeroes the refined counters on `stream`, then ONE launch.  The
 * survivors are appended to a context-owned [batch][keypoint capacity] refined buffer with [batch]
 * uint32 counters, allocated on first use (gdp_set_keypoint_capacity drops and reallocates it with
 * the keypoint buffer); outputs never exceed inputs, so it cannot overflow.  The device order is
 * unspecified.  The keypoint list itself is not changed, and gdp_detect_extrema leaves the refined
 * results alone: they stay those of the last refinement.  Arguments as for gdp_detect_extrema:
 * contrast_threshold >= 0 (not NaN), edge_ratio 0 or finite and >= 1, else GDP_ERR_ARG; row-band
 * contexts GDP_ERR_STATE; GDP_ERR_STATE too before a keypoint buffer exists (gdp_device_keypoints'
 * condition).  The pyramid is only read. */
int gdp_refine_keypoints(gdp_ctx* ctx, float contrast_threshold, float edge_ratio, void* stream);
/* Records the last refinement kept in image b (blocking; waits for the context's OWN stream; 0
 * before any refinement). */
int gdp_refined_count(gdp_ctx* ctx, int b, size_t* kept);
/* Copy min(kept, `capacity`) refined records of image b to `host` (blocking), sorted ascending by
 * (octave, scale, row, col), then by the bit patterns of (dscale, drow, dcol, interp, value, kind),
 * so host results are the same run to run.  *stored = records written (may be NULL). */
int gdp_download_refined(gdp_ctx* ctx, int b, gdp_keypoint_refined* host, size_t capacity, size_t* stored);
/* Zero-copy view for device consumers: image b's refined records (capacity records, the first
 * *count valid, device order) and its counter.  GDP_ERR_STATE before the first refinement. */
int gdp_device_refined(const gdp_ctx* ctx, int b, const gdp_keypoint_refined** records, const uint32_t** count);
/* Make host[0..n) image b's keypoint list and set its counter to n (blocking; allocates the
 * keypoint buffer if needed): the state restore for the list, as gdp_upload_pyramid is for the
 * pyramid, and the way to refine points of the caller's own.  Every record is validated on the
 * host — octave < octaves, scale in [1, S], row in [1, rows-2], col in [1, cols-2], kind +1 or -1
 * (`value` is not used), n <= the keypoint capacity; anything else is GDP_ERR_ARG and changes
 * nothing. */
int gdp_upload_keypoints(gdp_ctx* ctx, int b, const gdp_keypoint* host, size_t n);

/* ---- extension: keypoint orientation assignment on the device ---------------------------------
 * The SIFT step after localisation, done where the pyramid and the refined list already are (no
 * reference counterpart, no parity claim): a gradient-orientation histogram of the Gaussian level
 * around every refined record, whose peaks give the keypoint its angle(s).  The Gaussian levels are
 * not stored, but the pyramid keeps the last one in level S+2 and DoG_t = G_t - G_{t+1}, so G_s is a
 * suffix sum of levels the context holds; with the order of the additions fixed it is specified bit
 * for bit.  It reads levels s..S+2 of the CURRENT pyramid (own or bound) and writes nothing of the
 * context's: its state is an object of its own, gdp_orient, created from a const context.
 *
 * The rule.  Every operation is a separately rounded float32 operation: no contraction, denormals
 * kept, `/` and sqrtf IEEE-correct.  For a refined record (o, s, r, c) with 1 <= s <= S, 1 <= r <=
 * rows-2, 1 <= c <= cols-2 (a record that names no such sample is dropped before any address is
 * formed from it), with P[t] the levels of octave o; only the integer sample is used, dscale, drow
 * and dcol are copied through, not read:
 *   Gaussian level   L = P[S+2];  for t = S+1 down to s:  L = L + P[t]  (element by element; levels
 *                    below s are never read)
 *   window           radius R_s = (9 + s) / (s + 1) in integer division — ceil(3 * 1.5 * sigma_s) with
 *                    sigma_s = 2 / (s + 1), gdp_conv_taps' schedule: 5, 3, 3, 2, 2, ..., at least 1;
 *                    weights w_s[d2] = expf(-((float)d2 * k_s)), d2 = 0 .. 2 R_s^2, with
 *                    k_s = (float)((s+1)*(s+1)) / 18.0f, computed on the HOST with glibc expf and
 *                    uploaded, as the window taps are (gdp_orient_weights returns them)
 *   samples          (dr, dc) in [-R, R]^2, rr = r + dr, cc = c + dc; skipped when rr is outside
 *                    [1, rows-2] or cc outside [1, cols-2]; otherwise
 *                      gx = L[rr][cc+1] - L[rr][cc-1]      gy = L[rr+1][cc] - L[rr-1][cc]
 *                      m  = sqrtf(gx*gx + gy*gy)
 *                    !(m < INFINITY) (NaN or inf) rejects the whole record; !(m > 0.0f) skips the sample
 *   bin              no atan2.  The quadrant:  q = 0 when gx > 0 && gy >= 0, (ax, ay) = (gx, gy);
 *                    q = 1 when gx <= 0 && gy > 0, (ax, ay) = (gy, -gx);  q = 2 when gx < 0 && gy <= 0,
 *                    (ax, ay) = (-gx, -gy);  q = 3 otherwise, (ax, ay) = (-gy, gx).  j = the number of
 *                    k in 1..8 with ay >= ax * T[k], T[k] the float32 nearest to tan(k * 10 degrees):
 *                      T[1..8] = 0x3e348f0f 0x3eba5a4e 0x3f13cd3a 0x3f56cf3c
 *                                0x3f988b62 0x3fddb3d7 0x402fd6ac 0x40b57b24      (bit patterns)
 *                    bin = 9*q + j.  Angles run from the +col axis towards the +row axis:
 *                    (gx, gy) = (1,0) -> 0, (0,1) -> 9, (-1,0) -> 18, (0,-1) -> 27, (1,1) -> 4
 *   histogram        per window row dr a partial part_dr[36] starts at +0 and takes its samples in
 *                    ascending dc:  part[bin] = part[bin] + m * w_s[dr*dr + dc*dc];  then hist starts
 *                    at +0 and takes the rows in ascending dr:  hist[k] = hist[k] + part_dr[k]  (a
 *                    skipped row is a partial of +0; all terms are >= 0, so adding +0 is the identity)
 *   smoothing        indices mod 36:
 *                      h[k] = ((hist[k-2] + hist[k+2]) * 0.0625f + (hist[k-1] + hist[k+1]) * 0.25f)
 *                             + hist[k] * 0.375f
 *                    the record is rejected unless fabsf(h[k]) < INFINITY for every k
 *   peaks            mx = h[0]; for k = 1..35: if (h[k] > mx) mx = h[k];  thr = mx * 0.8f;  bin k is a
 *                    peak when h[k] > h[k-1] && h[k] > h[k+1] && h[k] >= thr; with l = h[k-1], rt = h[k+1]
 *                      b = (float)k + (0.5f * (l - rt)) / ((l - 2.0f*h[k]) + rt)
 *                      if (b < 0.0f) b = b + 36.0f;   if (b >= 36.0f) b = b - 36.0f;
 *                      angle = b * 10.0f                                   (degrees, [0, 360))
 * One output record per peak (a record without a peak — a flat window — yields none): the result is
 * an exact multiset. */
typedef struct gdp_keypoint_oriented {   /* 48 bytes, three 16-B stores */
    /* bytes 0..31: the input gdp_keypoint_refined, copied */
    uint16_t octave; uint8_t scale; int8_t kind; int32_t row, col; float value;
    float dscale, drow, dcol, interp;
    float angle;      /* degrees, [0, 360) */
    float peak;       /* h[k] of this peak */
    uint32_t bin;     /* k */
    uint32_t peaks;   /* records this input produced (>= 1) */
} gdp_keypoint_oriented;
typedef struct gdp_orient gdp_orient;
/* An orientation object bound to one whole-image context (a row band is GDP_ERR_STATE: the window
 * crosses band edges).  It owns the weight table, a [batch][capacity_per_image] output buffer with
 * [batch] uint32 counters and the caller's input lists; capacity_per_image = 0 means twice the
 * context's keypoint capacity at creation.  The context is only read — its pyramid, geometry and
 * refined list are looked up at every launch, so gdp_set_keypoint_capacity, gdp_set_output_device
 * and rebuilds in between are harmless — and must outlive the object: destroy the object first.
 * gdp_orient_last_error(w) describes w's last failure (w NULL: this thread's last failed create). */
int gdp_orient_create(gdp_orient** out, const gdp_ctx* ctx, size_t capacity_per_image);
void gdp_orient_destroy(gdp_orient* w);
const char* gdp_orient_last_error(const gdp_orient* w);
/* Make host[0..n) image b's input list instead of the context's refined list (blocking): the way
 * to orient points of the caller's own.  Every record is validated on the host as
 * gdp_upload_keypoints does (octave, scale in [1, S], row, col, kind), n <= the object's capacity;
 * anything else is GDP_ERR_ARG and changes nothing.  host = NULL goes back to the context's list. */
int gdp_orient_set_input(gdp_orient* w, int b, const gdp_keypoint_refined* host, size_t n);
/* Orient every image's list: zeroes the counters on `stream` (NULL = the context's own stream),
 * then ONE launch over all images; asynchronous and stream-ordered.  The input of an image is the
 * caller's list if one is set, else the first min(refined counter, keypoint capacity) records of the
 * context's refined list, read on the device — the host never reads that counter, so launching this
 * right after gdp_refine_keypoints on the same stream is the normal use.  GDP_ERR_STATE when an
 * image has neither a list of the caller's nor a refined buffer (gdp_device_refined's condition).
 * More records may be produced than the capacity holds: the counter still counts them all, the
 * buffer then holds exactly `capacity` true records (which ones is unspecified; a keypoint's
 * records need not all be among them) and nothing is stored at or beyond it.  The device order is
 * unspecified. */
int gdp_orient_keypoints(gdp_orient* w, void* stream);
/* Records the last orientation produced for image b (blocking; waits for the context's OWN stream;
 * 0 before any). */
int gdp_oriented_count(gdp_orient* w, int b, size_t* found);
/* Copy min(found, the object's capacity, `capacity`) records of image b to `host` (blocking), sorted
 * ascending by (octave, scale, row, col, bin), ties by the record's twelve 32-bit words compared as
 * unsigned in memory order, so host results are the same run to run.  *stored = records written,
 * *found = gdp_oriented_count (either may be NULL). */
int gdp_download_oriented(gdp_orient* w, int b, gdp_keypoint_oriented* host, size_t capacity,
                          size_t* stored, size_t* found);
/* Zero-copy view for device consumers: image b's records (capacity records, the first
 * min(*count, capacity) valid, device order) and its counter. */
int gdp_device_oriented(const gdp_orient* w, int b, const gdp_keypoint_oriented** records,
                        const uint32_t** count);
/* The window of scale s in a pyramid of S: weights[d2] = w_s[d2] for d2 = 0 .. 2R*R (at most 51
 * floats) and the radius R.  Pure host computation: no device, no context. */
int gdp_orient_weights(int S, int scale, float* weights /* 2R*R+1, at most 51 */, int* radius);

/* ---- extension: SIFT descriptors on the device ------------------------------------------------
 * The last step of the keypoint chain, done where the pyramid and the oriented list already are (no
 * reference counterpart, no parity claim): Lowe's 4 x 4 x 8 gradient histogram around every oriented
 * record, rotated to the keypoint's angle, normalised, clipped and quantised to 128 bytes — something
 * a caller can match without ever downloading the pyramid.  It reads levels s..S+2 of the CURRENT
 * pyramid (own or bound) and writes nothing of the context's or the orientation object's: its state
 * is an object of its own, gdp_describe, created from a const context and a const gdp_orient.
 *
 * The rule.  Every operation is a separately rounded float32 operation: no contraction, denormals
 * kept, `/` and sqrtf IEEE-correct; integer arithmetic is exact.  The result is an exact multiset of
 * 176-byte records.
 *   input            a gdp_keypoint_oriented record (o, s, r, c, angle).  It is dropped before any
 *                    address is formed from it unless 1 <= s <= S, 1 <= r <= rows-2, 1 <= c <= cols-2
 *                    and 0.0f <= angle && angle < 360.0f (a NaN angle drops it).  Only the integer
 *                    sample and `angle` are read; everything else is copied through
 *   Gaussian level   gdp_orient_keypoints' rule:  L = P[S+2];  for t = S+1 down to s:  L = L + P[t]
 *                    (levels below s are never read)
 *   window           radius R_s = (2121 + 50*(s+1)) / (100*(s+1)) in integer division — round(3 sigma_s
 *                    * sqrt(2) * 2.5) with sigma_s = 2 / (s + 1): 11, 7, 5, 4, 4, 3, 3, 2, 2 for
 *                    s = 1..9;  inv_s = (float)(s+1) / 6.0f, one over the bin width 3 sigma_s
 *   weights          W_s[d2] = expf(-((float)d2 * k_s)), d2 = 0 .. 2 R_s^2 (at most 243 entries), with
 *                    k_s = (float)((s+1)*(s+1)) / 288.0f: Lowe's Gaussian of sigma = 2 bins, a function
 *                    of the integer distance because a rotation keeps distances.  Computed on the HOST
 *                    with glibc expf and uploaded (gdp_describe_tables returns them); no exp on the device
 *   rotation         no sin or cos on the device: a table of 1,440 quarter-degree steps built on the
 *                    host.  Q[m] = (float)cos(m * pi / 720) evaluated in double, m = 0..360, with
 *                    Q[0] = 1 and Q[360] = 0 set exactly; for a = 360k + m, (C[a], S[a]) is
 *                    (Q[m], Q[360-m]) rotated k times by (c, s) -> (-s, c).
 *                      a = (int)(angle * 4.0f + 0.5f);  if (a >= 1440) a -= 1440;
 *                      ca = C[a],  sa = S[a]
 *   samples          (dr, dc) in [-R, R]^2, rr = r + dr, cc = c + dc; skipped when rr is outside
 *                    [1, rows-2] or cc outside [1, cols-2]; otherwise, with x = (float)dc, y = (float)dr
 *                      cb = ((x*ca + y*sa) * inv_s) + 1.5f
 *                      rb = ((y*ca - x*sa) * inv_s) + 1.5f
 *                    skipped unless rb > -1 && rb < 4 && cb > -1 && cb < 4; then
 *                      gx = L[rr][cc+1] - L[rr][cc-1]      gy = L[rr+1][cc] - L[rr-1][cc]
 *                      m  = sqrtf(gx*gx + gy*gy)
 *                    !(m < INFINITY) (NaN or inf) rejects the whole record; !(m > 0.0f) skips the sample
 *   orientation      no atan2.   gu = gx*ca + gy*sa     gv = gy*ca - gx*sa
 *                    the quadrant as in gdp_orient_keypoints' rule, applied to (gu, gv):  q = 0 when
 *                    gu > 0 && gv >= 0, (ax, ay) = (gu, gv);  q = 1 when gu <= 0 && gv > 0, (ax, ay) =
 *                    (gv, -gu);  q = 2 when gu < 0 && gv <= 0, (ax, ay) = (-gu, -gv);  q = 3 otherwise,
 *                    (ax, ay) = (-gv, gu).  Then
 *                      if (ay <= ax)  w8 = (ax > 0) ? A(ay / ax) : 0;   else  w8 = 2.0f - A(ax / ay);
 *                      ob = (float)(2*q) + w8;   if (ob >= 8.0f) ob = ob - 8.0f;
 *                    A(t) ~ atan(t) * 4 / pi on [0, 1] is an odd polynomial in Horner form: z = t*t;
 *                    p = c5;  p = p*z + c4;  ...  p = p*z + c0;  A = p*t  (each * and + rounded), with
 *                      c0..c5 = 0x3fa2f890 0xbed8d61d 0x3e7c5661 0xbe17cbe9 0x3d89486e 0xbc74784e
 *                    (bit patterns).  Over the float32 t of [0, 1] its error is at most 2.24e-6 bins
 *                    (1.0e-4 degrees), it is monotone, and A(1) = 0.99999785 < 1
 *   trilinear split  r0 = floorf(rb), c0 = floorf(cb), o0 = floorf(ob);  fr = rb - r0, fc = cb - c0,
 *                    fo = ob - o0;  mag = m * W_s[dr*dr + dc*dc].  As OpenCV splits:  v1 = mag*fr,
 *                    v0 = mag - v1;  each of those by fc the same way (vc1 = v*fc, vc0 = v - vc1);  each
 *                    of those by fo the same way.  The eight values go to bins
 *                    ((r0+i)*4 + (c0+j))*8 + ((o0+k) mod 8), i, j, k in {0, 1}; a value is dropped when
 *                    r0+i or c0+j is outside [0, 3].  All eight are >= +0 and their targets distinct
 *   histogram        gdp_orient_keypoints' order: per window row dr a partial part_dr[128] starts at +0
 *                    and takes its samples in ascending dc; hist starts at +0 and adds the partials in
 *                    ascending dr (a skipped row is a partial of +0: the identity, every term is >= 0).
 *                    The record is rejected unless hist[i] < INFINITY for every i
 *   normalisation    T(v), the tree sum of squares:  t[i] = v[i]*v[i];  for step = 64, 32, ..., 1:
 *                    t[i] = t[i] + t[i+step] for i < step;  T = t[0].
 *                      n  = sqrtf(T(hist));   rejected unless n > 0 && n < INFINITY
 *                      h[i] = hist[i] / n;    if (h[i] > 0.2f) h[i] = 0.2f
 *                      n2 = sqrtf(T(h))
 *                      qv = (h[i] / n2) * 512.0f
 *                      desc[i] = qv >= 255.0f ? 255 : (uint8_t)(int)qv
 * One output record per input that is neither dropped nor rejected. */
typedef struct gdp_keypoint_described {  /* 176 bytes, eleven 16-B stores */
    /* bytes 0..47: the input gdp_keypoint_oriented, copied */
    uint16_t octave; uint8_t scale; int8_t kind; int32_t row, col; float value;
    float dscale, drow, dcol, interp;
    float angle, peak; uint32_t bin, peaks;
    uint8_t desc[128];   /* [row bin][col bin][orientation bin] */
} gdp_keypoint_described;
typedef struct gdp_describe gdp_describe;
/* A descriptor object bound to one whole-image context (a row band is GDP_ERR_STATE: the window
 * crosses band edges) and, optionally, to the orientation object `src` of that context whose list it
 * describes (src = NULL: every image needs a list of the caller's, gdp_describe_set_input).  It owns
 * the weight and rotation tables, a [batch][capacity_per_image] output buffer with [batch] uint32
 * counters and the caller's input lists; capacity_per_image = 0 means src's capacity, or the
 * context's keypoint capacity at creation when src is NULL.  The context and src are only read —
 * looked up at every launch — and must outlive the object: destroy the object first.
 * gdp_describe_last_error(w) describes w's last failure (w NULL: this thread's last failed create). */
int gdp_describe_create(gdp_describe** out, const gdp_ctx* ctx, const gdp_orient* src, size_t capacity_per_image);
void gdp_describe_destroy(gdp_describe* w);
const char* gdp_describe_last_error(const gdp_describe* w);
/* Make host[0..n) image b's input list instead of src's oriented list (blocking): the way to describe
 * points of the caller's own.  Every record is validated on the host exactly as the device checks it
 * (octave, scale in [1, S], row, col, and 0 <= angle < 360, a NaN refused), n <= the object's
 * capacity; anything else is GDP_ERR_ARG and changes nothing.  host = NULL goes back to src's list. */
int gdp_describe_set_input(gdp_describe* w, int b, const gdp_keypoint_oriented* host, size_t n);
/* Describe every image's list: zeroes the counters on `stream` (NULL = the context's own stream),
 * then ONE launch over all images; asynchronous and stream-ordered.  The input of an image is the
 * caller's list if one is set, else the first min(oriented counter, src's capacity) records of src's
 * list, read on the device — the host never reads that counter, so launching this right after
 * gdp_orient_keypoints on the same stream is the normal use.  GDP_ERR_STATE when an image has neither
 * a list of the caller's nor a src.  Outputs never exceed inputs; with a smaller capacity the counter
 * still counts every record, the buffer then holds exactly `capacity` true records (which ones is
 * unspecified) and nothing is stored at or beyond it.  The device order is unspecified. */
int gdp_describe_keypoints(gdp_describe* w, void* stream);
/* Records the last description produced for image b (blocking; waits for the context's OWN stream;
 * 0 before any). */
int gdp_described_count(gdp_describe* w, int b, size_t* found);
/* Copy min(found, the object's capacity, `capacity`) records of image b to `host` (blocking), sorted
 * ascending by (octave, scale, row, col, bin), ties by the record's 44 32-bit words compared as
 * unsigned in memory order, so host results are the same run to run.  *stored = records written,
 * *found = gdp_described_count (either may be NULL). */
int gdp_download_described(gdp_describe* w, int b, gdp_keypoint_described* host, size_t capacity,
                           size_t* stored, size_t* found);
/* Zero-copy view for device consumers: image b's records (capacity records, the first
 * min(*count, capacity) valid, device order) and its counter. */
int gdp_device_described(const gdp_describe* w, int b, const gdp_keypoint_described** records,
                         const uint32_t** count);
/* The tables of scale s in a pyramid of S: weights[d2] = W_s[d2] for d2 = 0 .. 2R*R (at most 243
 * floats), the radius R, and the rotation table C[0..1440), S[0..1440) (the same for every scale).
 * Any output pointer but `radius` may be NULL.  Pure host computation: no device, no context. */
int gdp_describe_tables(int S, int scale, float* weights /* 2R*R+1, at most 243 */, int* radius,
                        float* cos1440, float* sin1440);

/* ---- extension: descriptor matching on the device ---------------------------------------------
 * What the descriptors are for: the nearest and second-nearest TRAIN descriptor of every QUERY
 * descriptor, brute force, where both lists already are (no reference counterpart, no parity claim).
 * The distance sweep runs on the i8 matrix cores, which accumulate in int32, so every distance is an
 * exact integer.  It writes nothing of a context, an orientation object or a describe object: its
 * state is an object of its own, gdp_match, created from two const gdp_describe objects.
 *
 * The rule.  Integers only, apart from the two marked float steps, where every operation is a
 * separately rounded float32 operation.  Two lists of gdp_keypoint_described records, the query
 * list Q[0..nq) and the train list T[0..nt):
 *   1 distance      dist(i, j) = sum over k < 128 of (Q[i].desc[k] - T[j].desc[k])^2, an exact
 *                   integer (at most 128 * 255^2 = 8,323,200)
 *   2 nearest       for query i the nearest train index is the j that minimises the pair
 *                   (dist(i, j), j) lexicographically: ties go to the lowest index.  `distance` is
 *                   its distance
 *   3 second        `second` is the minimum of dist(i, j') over j' != j; it may equal `distance`.
 *                   With nt = 1 it is 0xffffffff.  With nt = 0 the query yields nothing
 *   4 ratio (float) when ratio != 0:  r2 = ratio * ratio (one rounded product);  keep when
 *                   (float)distance < r2 * (float)second  (one rounded product, one comparison).
 *                   (float)0xffffffff is 2^32; every real distance is below 2^24, so its conversion
 *                   is exact
 *   5 cap           keep when distance <= max_distance; 0xffffffff means no cap
 *   6 mutual        when mutual != 0, keep only if i is the nearest query of train j under the same
 *                   rule with the sides swapped: i minimises (dist(i', j), i') over i'
 *   7 coordinates   (float) for a record, sc = (float)(1u << (octave & 31)),
 *                   x = ((float)col + dcol) * sc,  y = ((float)row + drow) * sc
 *   8 addresses     nothing is read from a record except octave, row, col, drow, dcol and desc, and
 *                   no address is formed from record contents: any 176 bytes are a valid record
 * At most one output record per query.  Every quantity is a function of the two lists with a total
 * order for ties, so the result is an exact set, independent of tiling, chunking and wave timing.
 * `query` and `train` index the lists in the order the kernel read them — the device order
 * (gdp_device_described), which is unspecified for a list the pipeline produced and exactly the
 * caller's for a list the caller supplied (gdp_match_set_input).  The coordinates are what a caller
 * uses when they do not want to resolve indices. */
typedef struct gdp_match_record {   /* 32 bytes, two 16-B stores */
    uint32_t query, train;          /* indices into the lists as the kernel read them */
    uint32_t distance, second;
    float qx, qy, tx, ty;           /* image coordinates of the two keypoints */
} gdp_match_record;
typedef struct gdp_match gdp_match;
/* A match object reading two describe objects (both non-NULL; they may be the same object, and may
 * belong to different contexts, but must be on the same device, else GDP_ERR_ARG).  A capacity of 0
 * means that object's capacity; neither may exceed 2^30.  The object owns an output buffer of
 * query_capacity records, one uint32 counter, its scratch and the caller's lists.  Both describe
 * objects are only read — looked up at every launch — and must outlive the match object: destroy it
 * first.  gdp_match_last_error(m) describes m's last failure (m NULL: this thread's last failed
 * create). */
int gdp_match_create(gdp_match** out, const gdp_describe* query, const gdp_describe* train, size_t query_capacity,
                     size_t train_capacity);
void gdp_match_destroy(gdp_match* m);
const char* gdp_match_last_error(const gdp_match* m);
/* Make host[0..n) the list of `side` (0 query, 1 train) instead of the describe object's (blocking):
 * n must not exceed that side's capacity, else GDP_ERR_ARG and nothing changes.  Records are not
 * validated (point 8 of the rule).  An empty list (host non-NULL, n = 0) is a list; host = NULL goes
 * back to the describe object's list. */
int gdp_match_set_input(gdp_match* m, int side, const gdp_keypoint_described* host, size_t n);
/* Match: zeroes the counter on `stream` (NULL = the QUERY context's own stream), then launches;
 * asynchronous and stream-ordered.  When the train context's work runs on another stream the caller
 * orders it.  A side without a list of the caller's reads the first min(counter, the describe
 * object's capacity, that side's capacity) records of image query_image / train_image of its
 * describe object; the count is read on the device, the host never reads it, so launching this right
 * after gdp_describe_keypoints on the same stream is the normal use.  Outputs never exceed nq, so
 * the buffer cannot overflow.  `ratio` is 0 (no ratio test) or in (0, 1]; a NaN or anything else is
 * GDP_ERR_ARG, and so is an image index out of range.  The device order is unspecified. */
int gdp_match_descriptors(gdp_match* m, int query_image, int train_image, float ratio, uint32_t max_distance,
                          int mutual, void* stream);
/* Records the last match produced (blocking; waits for the query context's OWN stream; 0 before any). */
int gdp_match_count(gdp_match* m, size_t* found);
/* Copy min(found, `capacity`) records to `host` (blocking), sorted ascending by `query`, which is
 * unique per record.  *stored = records written, *found = gdp_match_count (either may be NULL). */
int gdp_download_matches(gdp_match* m, gdp_match_record* host, size_t capacity, size_t* stored, size_t* found);
/* Zero-copy view for device consumers: the records (query_capacity records, the first *count valid,
 * device order) and the counter. */
int gdp_device_matches(const gdp_match* m, const gdp_match_record** records, const uint32_t** count);
/* How the object cuts the work (any output may be NULL): its two capacities; the chunk granule; and
 * the number of chunks of the train list (one grid dimension of the distance sweep) and of the query
 * list (the swapped sweep of the mutual test).  A list of n records in c chunks is cut at multiples of
 * ceil(ceil(n / c) / granule) * granule, computed on the device from the count it reads. */
int gdp_match_layout(const gdp_match* m, size_t* query_capacity, size_t* train_capacity, uint32_t* chunk_unit,
                     uint32_t* train_chunks, uint32_t* query_chunks);

/* ---- extension: RANSAC homography of the matches on the device ---------------------------------
 * What the matches' coordinates are for: which matches are geometrically consistent, and under which
 * projective transform (no reference counterpart, no parity claim).  H hypotheses, each the exact
 * homography of four sampled matches, are scored against every match; the best one is the model and
 * the matches it accepts are the inliers.  It writes nothing of a context, an orientation, describe
 * or match object: its state is an object of its own, gdp_ransac, created from a const gdp_match.
 *
 * The rule.  Input is a list M[0..n) of gdp_match_record, of which only qx, qy, tx, ty are read; the
 * parameters are `hypotheses` H, `seed`, `threshold` t and `min_inliers`.
 *   1 sample        (integers only.)  mix(x) on uint32 with wrap-around:  x ^= x >> 16;
 *                   x *= 0x7feb352d;  x ^= x >> 15;  x *= 0x846ca68b;  x ^= x >> 16.  For hypothesis
 *                   h < H and slot k < 4:  r = mix(seed + 0x9e3779b9 * (4h + k + 1))  and
 *                   sample[k] = ((uint64)r * n) >> 32.  A hypothesis is VALID only when n >= 4 and
 *                   its four indices are pairwise distinct; there is no resampling loop
 *   2 basis         (float64, every operation separately rounded, no contraction.)  The four query
 *                   points, converted exactly to double, are p_k = (x_k, y_k, 1), and Mq = [p0 p1 p2]
 *                   has them as its COLUMNS: Mq[0][c] = x_c, Mq[1][c] = y_c, Mq[2][c] = 1.  adj(M) is
 *                   nine expressions, each two rounded products and one rounded difference:
 *                     adj[0][0] = M[1][1] * M[2][2] - M[1][2] * M[2][1]
 *                     adj[0][1] = M[0][2] * M[2][1] - M[0][1] * M[2][2]
 *                     adj[0][2] = M[0][1] * M[1][2] - M[0][2] * M[1][1]
 *                     adj[1][0] = M[1][2] * M[2][0] - M[1][0] * M[2][2]
 *                     adj[1][1] = M[0][0] * M[2][2] - M[0][2] * M[2][0]
 *                     adj[1][2] = M[0][2] * M[1][0] - M[0][0] * M[1][2]
 *                     adj[2][0] = M[1][0] * M[2][1] - M[1][1] * M[2][0]
 *                     adj[2][1] = M[0][1] * M[2][0] - M[0][0] * M[2][1]
 *                     adj[2][2] = M[0][0] * M[1][1] - M[0][1] * M[1][0]
 *                   lambda = adj(Mq) * p3:  lambda[r] = (adj[r][0] * x3 + adj[r][1] * y3) + adj[r][2];
 *                   A[r][c] = Mq[r][c] * lambda[c].  The same from the four train points gives B.  No
 *                   division and no pivoting anywhere
 *   3 compose       (float64.)  J = adj(A) as above;
 *                   G[r][c] = (B[r][0] * J[0][c] + B[r][1] * J[1][c]) + B[r][2] * J[2][c]
 *   4 normalise     s = max |G[r][c]|.  If s is 0, infinite or NaN, or any entry is NaN, the hypothesis
 *                   is INVALID.  Otherwise s = m * 2^e with m in [0.5, 1) (frexp) and G <- ldexp(G, -e);
 *                   w0 = (G[2][0] * x0 + G[2][1] * y0) + G[2][2] at query sample 0, in double; if
 *                   w0 < 0, G is negated;  h[3r + c] = (float)G[r][c], round to nearest even, float32
 *                   denormals kept (so max |h| lies in [0.5, 1]: a value just below 1 may round to 1).
 *                   An invalid hypothesis has h[] = 0 and counts nothing; its sample[] is stored all
 *                   the same
 *   5 score         (float32, every operation separately rounded.)  For match i = (x, y, X, Y):
 *                     u = (h0 * x + h1 * y) + h2,  v = (h3 * x + h4 * y) + h5,  w = (h6 * x + h7 * y) + h8,
 *                     dx = X * w - u,  dy = Y * w - v,  e = dx * dx + dy * dy;
 *                   an inlier when  w > 0  and  e <= (t * t) * (w * w).  No division; NaN coordinates fail
 *                   both comparisons.  The hypothesis's count is the number of inliers among i < n, an
 *                   exact integer
 *   6 select        the winner is the valid hypothesis with the largest count, ties to the lowest h.  A
 *                   model exists iff a winner exists and its count >= max(min_inliers, 4)
 *   7 inliers       the records of M that step 5 accepts under the winner's h[], copied unchanged; the
 *                   empty list when no model exists
 *   8 addresses     nothing but the four floats is read from a record, and no address is formed from
 *                   record contents: any 32 bytes are a valid record
 * Every quantity is a function of the list in the order the kernel read it, the seed and the
 * parameters, and the counts are integer sums, so the result is an exact set, independent of tiling
 * and wave timing.  For a list the pipeline produced (the match object's) that order is the device
 * order (gdp_device_matches), which is unspecified, as with `query` / `train` of the matches; for a
 * list the caller supplied (gdp_ransac_set_input) it is exactly the caller's.  The model is the
 * exact homography of four matches; gdp_refit_homography (below) refits it over the inliers by least
 * squares.  Out of scope: early termination, other models. */
typedef struct gdp_homography {   /* 64 bytes, four 16-B stores */
    float    h[9];                /* row-major, as scored: max |h| in [0.5, 1]; all 0 = invalid / none */
    uint32_t hypothesis;          /* its index; 0xffffffff in the model record when there is none */
    uint32_t inliers;             /* step 5's count (0 in a model record without a model) */
    uint32_t matches;             /* the n this launch read */
    uint32_t sample[4];           /* step 1's indices; 0xffffffff in a model record without a model */
} gdp_homography;
typedef struct gdp_ransac gdp_ransac;
/* A fit object reading one match object (non-NULL), which is only read — its list and counter are
 * looked up at every launch — and must outlive this object: destroy this one first.  `capacity` is
 * the longest list a fit reads (0: the match object's query capacity; at most 2^30), max_hypotheses
 * the most hypotheses of one fit (0: 4,096; above 65,536 is GDP_ERR_ARG).  The object owns the
 * hypothesis records, an inlier buffer of `capacity` records (so it cannot overflow), the model
 * record, one uint32 counter and the caller's list.  gdp_ransac_last_error(r) describes r's last
 * failure (r NULL: this thread's last failed create). */
int gdp_ransac_create(gdp_ransac** out, const gdp_match* src, size_t capacity, uint32_t max_hypotheses);
void gdp_ransac_destroy(gdp_ransac* r);
const char* gdp_ransac_last_error(const gdp_ransac* r);
/* Make host[0..n) the list instead of the match object's (blocking): n must not exceed the capacity,
 * else GDP_ERR_ARG and nothing changes.  Records are not validated (point 8 of the rule).  An empty
 * list (host non-NULL, n = 0) is a list; host = NULL goes back to the match object's list. */
int gdp_ransac_set_input(gdp_ransac* r, const gdp_match_record* host, size_t n);
/* Fit: zeroes the counter on `stream` (NULL = the query context's own stream), then launches;
 * asynchronous and stream-ordered.  Without a list of the caller's it reads the first min(counter,
 * the match object's query capacity, this object's capacity) records of the match object's output;
 * the count is read on the device, the host never reads it, so launching this right after
 * gdp_match_descriptors on the same stream is the normal use.  `hypotheses` must be in
 * 1..max_hypotheses and `threshold` finite and >= 0 (a NaN included), else GDP_ERR_ARG and nothing
 * changes: the previous fit's results stay downloadable. */
int gdp_fit_homography(gdp_ransac* r, uint32_t hypotheses, uint32_t seed, float threshold,
                       uint32_t min_inliers, void* stream);
/* Inliers of the last fit (blocking; waits for the query context's OWN stream; 0 before any). */
int gdp_ransac_count(gdp_ransac* r, size_t* inliers);
/* The model record of the last fit (blocking): the winner's record, or h[] = 0, hypothesis =
 * 0xffffffff, inliers = 0, matches = n, sample[] = 0xffffffff when there is no model (matches = 0
 * before any fit). */
int gdp_download_homography(gdp_ransac* r, gdp_homography* model);
/* Records 0 .. H-1 of the last fit, in index order, as many as fit into `capacity` (blocking).
 * *stored = records written (may be NULL); 0 before any fit. */
int gdp_download_hypotheses(gdp_ransac* r, gdp_homography* host, size_t capacity, size_t* stored);
/* Copy min(found, `capacity`) inlier records to `host` (blocking), sorted ascending by `query`; a
 * buffer shorter than the list takes the head of the full sorted list.  *stored = records written,
 * *found = gdp_ransac_count (either may be NULL). */
int gdp_download_inliers(gdp_ransac* r, gdp_match_record* host, size_t capacity, size_t* stored, size_t* found);
/* Zero-copy view for device consumers (any output may be NULL): the inlier records (`capacity`
 * records, the first *count valid, device order), the counter and the model record. */
int gdp_device_inliers(const gdp_ransac* r, const gdp_match_record** records, const uint32_t** count,
                       const gdp_homography** model);
/* How the object cuts the work (any output may be NULL): its capacity and max_hypotheses; the chunk
 * granule of the match list (the scoring sweep cuts a list of n records into c chunks at multiples of
 * ceil(ceil(n / c) / granule) * granule, computed on the device from the count it reads); and the
 * hypotheses per block of the scoring sweep, one per lane. */
int gdp_ransac_layout(const gdp_ransac* r, size_t* capacity, uint32_t* max_hypotheses,
                      uint32_t* match_tile, uint32_t* hypothesis_tile);

/* ---- extension: least-squares refit of the fitted homography on the device ----------------------
 * What every user of a RANSAC homography does next: the model above is the exact map of four sampled
 * matches, and the algebraic least-squares homography of ALL its inliers is far closer to the true
 * one.  It is a second entry point on the fit object: it replaces the model record and the inlier
 * list IN PLACE, stream-ordered behind gdp_fit_homography, so gdp_warp_image, gdp_match_guided,
 * gdp_download_homography, gdp_download_inliers and gdp_device_inliers consume the refit model
 * unchanged and the host reads nothing.  A float reduction over thousands of records has no fixed
 * order; this one is done in exact integers, so the result is an exact set like the fit's.
 *
 * The rule.  M[0..n) is the list as the fit resolves it at launch (the caller's, else the first
 * min(counter, capacities) records of the match object), L the object's inlier list as it stands, m
 * the model record, t the `threshold`.  When m says "none" (hypothesis == 0xffffffff) every round
 * does nothing and status = 6.  Otherwise each of the `rounds` rounds runs:
 *   1 quantise      (integers.)  A record of L is USED when each of qx, qy, tx, ty is finite with
 *                   |f| < 16384, else SKIPPED.  q[k] = (int64)rint(f[k] * 256.0f), k = x, y, X, Y: the
 *                   float32 product is exact and rint is to nearest even
 *   2 origin        o[k] = floor(sum q[k] / used) over the used records, rounding toward -infinity.
 *                   Fewer than 4 used records: NO CANDIDATE (status 2; kq, kt, origin, h are 0)
 *   3 moments       (exact signed 128-bit integers.)  c = q - o.  With mono = (1, cx, cy, cx*cx, cx*cy,
 *                   cy*cy) indexed a = 0..5 and tmono = (1, cX, cY, cX*cX + cY*cY) indexed b = 0..3,
 *                   mu[a][b] = sum over the used records of mono[a] * tmono[b]: 24 sums.  |c| < 2^23, so
 *                   a term is < 2^93 and a sum of at most 2^30 terms < 2^123
 *   4 scale         kq = the smallest k >= 0 with mu[3][0] + mu[5][0] < used * 4^k, kt the same from
 *                   mu[0][3]: integer comparisons.  deg_q = (0, 1, 1, 2, 2, 2)[a], deg_t = (0, 1, 1, 2)[b]
 *   5 solve         (float64, every + - * / separately rounded, no contraction, no sqrt.)
 *                   S[a][b] = ldexp(+-((double)hi64 * 2^64 + (double)lo64), -(kq * deg_q + kt * deg_t)),
 *                   hi64 and lo64 the halves of |mu[a][b]| converted to nearest even, the sign mu's.
 *                   The unknown is g[0..8) with g8 = 1 in the normalised frame, the rows of the
 *                   inhomogeneous DLT being  x g0 + y g1 + g2 - X x g6 - X y g7 = X  and
 *                   x g3 + y g4 + g5 - Y x g6 - Y y g7 = Y.  The lower triangle of the 8 x 8 normal matrix
 *                   N (every entry not listed is +0) and the right-hand side:
 *                     P = [S[3][0] S[4][0] S[1][0]; S[4][0] S[5][0] S[2][0]; S[1][0] S[2][0] S[0][0]];
 *                     N[i][j] = N[3+i][3+j] = P[i][j] for j <= i < 3;  for (b, c) = (1, 0) and (2, 3):
 *                     N[6][c] = -S[3][b], N[6][c+1] = -S[4][b], N[6][c+2] = -S[1][b],
 *                     N[7][c] = -S[4][b], N[7][c+1] = -S[5][b], N[7][c+2] = -S[2][b],
 *                     rhs[c] = S[1][b], rhs[c+1] = S[2][b], rhs[c+2] = S[0][b];
 *                     N[6][6] = S[3][3], N[7][6] = S[4][3], N[7][7] = S[5][3], rhs[6] = -S[1][3], rhs[7] = -S[2][3]
 *                   LDL^T without pivoting, nothing skipped for being zero: for j = 0..7:
 *                     v[k] = L[j][k] * D[k] for k < j;  d = N[j][j], then d = d - L[j][k] * v[k] for
 *                     k = 0..j-1 ascending;  D[j] = d;  a pivot that is not > 0 (a NaN included) gives NO
 *                     CANDIDATE (status 3);  for i = j+1..7: e = N[i][j], then e = e - L[i][k] * v[k] for
 *                     k ascending;  L[i][j] = e / d
 *                   forward, i = 0..7: z[i] = rhs[i], then z[i] = z[i] - L[i][k] * z[k] for k = 0..i-1
 *                   ascending;  back, i = 7..0: g[i] = z[i] / D[i], then g[i] = g[i] - L[k][i] * g[k] for
 *                   k = i+1..7 ascending
 *   6 denormalise   (float64.)  a = 2^(8-kq), bx = ldexp(-(double)o[x], -kq), by likewise from o[y],
 *                   sc = 2^(kt-8), tX = (double)o[X] / 256, tY = (double)o[Y] / 256: all exact.  With
 *                   Hh = [g0 g1 g2; g3 g4 g5; g6 g7 1]:
 *                     K[r][0] = Hh[r][0] * a,  K[r][1] = Hh[r][1] * a,
 *                     K[r][2] = (Hh[r][0] * bx + Hh[r][1] * by) + Hh[r][2];
 *                     G[0][c] = sc * K[0][c] + tX * K[2][c],  G[1][c] = sc * K[1][c] + tY * K[2][c],
 *                     G[2][c] = K[2][c]
 *                   then step 4 of the fit rule without its sign step (w at the list's origin is g8 = 1):
 *                   s = max |G|; s 0, infinite or NaN, or a NaN entry: NO CANDIDATE (status 4);
 *                   else G <- ldexp(G, -e) with s = mant * 2^e (frexp) and h[3r + c] = (float)G[r][c]
 *   7 accept        c_cur and c_new are the fit rule's step-5 counts of m.h and of the candidate over M
 *                   under t (c_new = 0 without a candidate).  The candidate is ACCEPTED iff it exists,
 *                   c_new >= c_cur and c_new >= 4 (status 1; else, with a candidate, status 5).  On
 *                   acceptance m.h <- the candidate, m.inliers <- c_new, m.matches <- n, and L <- the records
 *                   of M that step 5 accepts under it; `hypothesis` and `sample[]` keep the RANSAC winner's
 *                   values.  Otherwise nothing changes, and the later rounds do nothing
 * As in the fit, nothing but the four floats is read from a record and no address is formed from record
 * contents.  The sweeps over L and M use min(1024, ceil(capacity / 2048)) blocks of 256 threads. */
typedef struct gdp_refit_record {   /* 96 bytes, six 16-B stores; all 0 before any refit */
    uint32_t rounds;              /* rounds requested */
    uint32_t accepted;            /* rounds accepted */
    uint32_t used, skipped;       /* step 1's counts in the last round that ran */
    uint32_t count_before;        /* the first round's c_cur */
    uint32_t count_after;         /* the model record's `inliers` at the end */
    uint32_t status;              /* of the last round that ran: 1 accepted, 2 too few used records, 3 pivot,
                                     4 non-finite, 5 fewer inliers than the model, 6 no model */
    uint32_t kq, kt;              /* step 4's exponents of the last candidate */
    int32_t  origin[4];           /* step 2's o[x, y, X, Y] of the last candidate, in 1/256 px */
    float    h[9];                /* the last candidate as scored, accepted or not (all 0: none) */
    uint32_t reserved[2];         /* 0 */
} gdp_refit_record;
/* Refit: asynchronous and stream-ordered on `stream` (NULL = the query context's own stream), behind
 * the gdp_fit_homography whose result it replaces; the host reads nothing.  `rounds` must be in 1..8
 * and `threshold` finite and >= 0, else (a NaN included) GDP_ERR_ARG and nothing changes.  The
 * refit's buffers are allocated by the object's first refit: that one call allocates device memory,
 * which synchronises the device, so it cannot be made under stream capture; make one refit before
 * capturing.  A later gdp_fit_homography gives what it gives without a refit; the refit record stays
 * that of the last refit. */
int gdp_refit_homography(gdp_ransac* r, uint32_t rounds, float threshold, void* stream);
/* The record of the last refit (blocking; all 0 before any). */
int gdp_download_refit(gdp_ransac* r, gdp_refit_record* rec);
/* Zero-copy view for device consumers: the record.  GDP_ERR_STATE before the first refit. */
int gdp_device_refit(const gdp_ransac* r, const gdp_refit_record** rec);

/* ---- extension: homography warp of an input image on the device ---------------------------------
 * What the homography is for: one image resampled into the other's frame under the fitted model,
 * stream-ordered behind the fit, with a measure of how well the two now agree (no reference
 * counterpart, no parity claim).  The output is an image in the source context's input format, so a
 * further context can bind it with gdp_set_input_device* and build a pyramid of the registered
 * image.  It writes nothing of a context, an orientation, describe, match or ransac object: its state
 * is an object of its own, gdp_warp, created from a const gdp_ransac.
 *
 * The rule.  Inputs: a model of nine float32 h[0..9), row-major, mapping query image coordinates
 * (x, y) to train image coordinates as gdp_fit_homography produces it — x is the column index and y
 * the row index of the octave-0 image, the convention of gdp_match_record; a SOURCE image (Hs x Ws,
 * int32 or uint8); a DESTINATION FRAME image (Hd x Wd); an int32 `fill`; a `direction`:
 *   GDP_WARP_TRAIN_TO_QUERY (0)  source = image train_image of the train context, destination frame =
 *                                image query_image of the query context, M = h
 *   GDP_WARP_QUERY_TO_TRAIN (1)  source = the query image, destination frame = the train image, M = the
 *                                normalised adjugate of h (step 1)
 *   1 matrix        (one thread, float64, every operation separately rounded, no division.)  When the
 *                   model record says "none" (hypothesis == 0xffffffff) there is NO MODEL: m[] = 0,
 *                   model = 0, every output pixel is `fill`, covered = 0, sad = 0.  Direction 0:
 *                   m[k] = h[k] unchanged and model = 1, whatever the bytes are.  Direction 1: G = adj(h)
 *                   with the nine expressions exactly as step 2 of the RANSAC rule writes them, h
 *                   converted exactly to double;
 *                     det = (h[0] * adj[0][0] + h[1] * adj[1][0]) + h[2] * adj[2][0];
 *                   s = max |G[r][c]|.  If s is 0, infinite or NaN, or any entry is NaN, or det is 0 or
 *                   NaN, there is no model (as above).  Otherwise s = mant * 2^e with mant in [0.5, 1)
 *                   (frexp) and G <- ldexp(G, -e); G is negated when det < 0 (the pre-image of a point
 *                   has positive w under h exactly when w' has det's sign, so after the negation the
 *                   same w > 0 test serves both directions);  m[3r + c] = (float)G[r][c], round to
 *                   nearest even, denormals kept
 *   2 sample        (float32, every operation separately rounded, no contraction, denormals kept.)
 *                   For output pixel (r, c), r < Hd, c < Wd:  x = (float)c,  y = (float)r,
 *                     u = (m0 * x + m1 * y) + m2,  v = (m3 * x + m4 * y) + m5,  w = (m6 * x + m7 * y) + m8.
 *                   If !(w > 0) the pixel is UNCOVERED.  sx = u / w, sy = v / w: two IEEE correctly
 *                   rounded divisions.  The pixel is COVERED iff
 *                     sx >= 0 && sy >= 0 && sx <= (float)(Ws - 1) && sy <= (float)(Hs - 1);  a NaN fails
 *   3 interpolate   (covered pixels only.)  x0f = floorf(sx), y0f = floorf(sy);  x0 = (int)x0f,
 *                   y0 = (int)y0f;  x1 = min(x0 + 1, Ws - 1),  y1 = min(y0 + 1, Hs - 1);
 *                   fx = sx - x0f,  fy = sy - y0f;  pAB = (float)source[yA][xB] (int -> float, round to
 *                   nearest even);
 *                     top = p00 + fx * (p01 - p00),  bot = p10 + fx * (p11 - p10),
 *                     val = top + fy * (bot - top),  q = rintf(val) (ties to even).
 *                   int32 output: INT32_MAX when q >= 2147483648.0f, INT32_MIN when
 *                   q < -2147483648.0f, else (int32_t)q.  uint8 output: clamped to 0..255.  The output
 *                   format is the SOURCE context's input format
 *   4 uncovered     pixels store `fill` (int32 output), or `fill` clamped to 0..255 (uint8 output)
 *   5 statistics    `covered` is the number of covered pixels; `sad` is the sum over covered pixels of
 *                   |out - dest[r][c]| as an exact uint64 integer sum, both read as integers whatever
 *                   the two formats are.  Both are integer sums, so the result is independent of tiling
 *                   and wave timing
 *   6 addresses     no address is formed from anything but indices the coverage test has bounded: any
 *                   nine floats and any pixel bytes are valid input
 * Refusals: a row-band context is GDP_ERR_STATE; a destination frame of Hd * Wd >= 2^32 pixels, an
 * image side above 16,777,216 (where (float)(Ws - 1) stops being exact), an image index out of range
 * or a direction other than 0 / 1 are GDP_ERR_ARG, and nothing changes.  Out of scope: other
 * interpolation kernels, anti-aliasing under minification, colour. */
enum { GDP_WARP_TRAIN_TO_QUERY = 0, GDP_WARP_QUERY_TO_TRAIN = 1 };
typedef struct gdp_warp_record {   /* 64 bytes */
    float    m[9];                 /* the matrix step 2 used; all 0 without a model */
    uint32_t model;                /* 1 / 0 */
    uint32_t covered, pixels;      /* pixels = Hd * Wd of this launch */
    uint64_t sad;
    uint32_t direction, reserved;  /* reserved = 0 */
} gdp_warp_record;
typedef struct gdp_warp gdp_warp;
/* A warp object reading one fit object (non-NULL) and, through its match object, the query and the
 * train context: all are only read — the model record and the two input images (what
 * gdp_device_input reports: the context's own buffer or a bound one) are looked up at every launch —
 * and must outlive this object: destroy this one first.  The object owns one output buffer large
 * enough for either direction in either format, the record and the caller's matrix.
 * gdp_warp_last_error(w) describes w's last failure (w NULL: this thread's last failed create). */
int gdp_warp_create(gdp_warp** out, const gdp_ransac* src);
void gdp_warp_destroy(gdp_warp* w);
const char* gdp_warp_last_error(const gdp_warp* w);
/* Make h9[0..9) the model instead of the fit's model record (blocking).  The floats are not
 * validated (point 6 of the rule); a caller's matrix is always a model in direction 0.  NULL goes
 * back to the fit's model record. */
int gdp_warp_set_model(gdp_warp* w, const float* h9);
/* Warp: asynchronous and stream-ordered (NULL = the QUERY context's own stream).  The model record is
 * read on the device, the host never reads it, so launching this right after gdp_fit_homography on
 * the same stream is the normal use.  When the train context's input was written on another stream
 * the caller orders it.  The output has the destination frame's size, the source context's input
 * format and a row pitch of the width rounded up to 4 elements. */
int gdp_warp_image(gdp_warp* w, int direction, int query_image, int train_image, int32_t fill, void* stream);
/* The record of the last launch (blocking; waits for the query context's OWN stream; all 0 before any). */
int gdp_download_warp_record(gdp_warp* w, gdp_warp_record* rec);
/* The last launch's Hd x Wd output to host rows of `pitch_elements` elements of the output format
 * (blocking); a pitch below Wd is GDP_ERR_ARG.  Nothing is copied before the first launch. */
int gdp_download_warped(gdp_warp* w, void* host, size_t pitch_elements);
/* Zero-copy view for device consumers (any output may be NULL): the output's first pixel, its pitch in
 * elements — one gdp_set_input_device / gdp_set_input_device_u8 accept for a context of *height x
 * *width in *format (GDP_INPUT_I32 / GDP_INPUT_U8) — and the record.  0 x 0 before the first launch. */
int gdp_device_warped(const gdp_warp* w, const void** pixels, size_t* pitch, int* height, int* width,
                      int* format, const gdp_warp_record** record);
/* How the sweep cuts the destination frame (any output may be NULL): the rows and columns of a wave's
 * tile and the consecutive columns one lane computes; a block is 2 x 2 such tiles. */
int gdp_warp_layout(const gdp_warp* w, uint32_t* tile_rows, uint32_t* tile_cols, uint32_t* pixels_per_lane);

/* ---- extension: guided matching under the fitted homography on the device ------------------------
 * What the homography is for on the matching side: with the model known, the partner of a query can
 * only lie near its projection, so the two lists are matched again inside a window round it — a few
 * candidates per query instead of the whole train list, and no ratio test needed to reject a wrong
 * match (no reference counterpart, no parity claim).  It writes nothing of a context, an orientation,
 * describe, match or ransac object: its state is an object of its own, gdp_guided, created from a
 * const gdp_ransac.
 *
 * The rule.  Inputs: the two lists of gdp_keypoint_described records that the match object behind the
 * fit reads, Q[0..nq) and T[0..nt), resolved for query_image / train_image exactly as
 * gdp_match_descriptors resolves them; nine float32 h[0..9), row-major, mapping query (x, y) to train
 * coordinates (the fit's model record, or the caller's floats); the parameters `radius` r, `ratio`,
 * `max_distance` and `unique`.
 *   1 coordinates   (float32.)  Step 7 of the match rule for both lists: (qx, qy) and (tx, ty)
 *   2 projection    (float32, every operation separately rounded, no contraction, denormals kept.)
 *                     u = (h0 * qx + h1 * qy) + h2,  v = (h3 * qx + h4 * qy) + h5,  w = (h6 * qx + h7 * qy) + h8.
 *                   A query with !(w > 0) has NO WINDOW and yields nothing.  sx = u / w, sy = v / w: two
 *                   IEEE correctly rounded divisions.  The fit's "none" record has h[] = 0, so w = 0 and
 *                   nothing is output: no flag is read
 *   3 window        (float32, one rounded operation each.)  x0 = sx - r, x1 = sx + r, y0 = sy - r, y1 = sy + r
 *   4 candidates    train j is a candidate of query i iff
 *                     x0 <= tx_j && tx_j <= x1 && y0 <= ty_j && ty_j <= y1:
 *                   four comparisons and nothing else, so a NaN anywhere fails.  The window is a square
 *                   on purpose: a predicate made only of comparisons is what a cell search can be
 *                   exactly conservative for
 *   5 nearest       dist(i, j) is step 1 of the match rule, an exact integer.  The nearest train of
 *                   query i minimises (dist(i, j), j) lexicographically over its candidates; `second` is
 *                   the minimum of dist over its other candidates, 0xffffffff with a single candidate.  A
 *                   query without a candidate yields no record
 *   6 ratio, cap    steps 4 and 5 of the match rule unchanged.  A query with a single candidate passes
 *                   the ratio test: (float)0xffffffff is 2^32
 *   7 unique        when unique != 0: of the records surviving step 6 that share a `train` index, only
 *                   the one that minimises (distance, query) lexicographically stays; a loser is absent,
 *                   it is not matched again.  The output is then one-to-one.  (This stands where the
 *                   dense matcher has its mutual test, whose swapped search has no exact windowed form.)
 *   8 addresses     nothing is read from a record except octave, row, col, drow, dcol and desc: any 176
 *                   bytes are a valid record, and any nine floats a valid h.  A cell index formed from
 *                   coordinates is clamped into the grid in float before the conversion to integer, and a
 *                   train with a NaN coordinate is in no cell, because it can be nobody's candidate
 * At most one gdp_match_record per query, filled as the match rule fills it.  Every quantity is a
 * function of the two lists, h and the parameters with a total order for ties, so the result is an
 * exact set, independent of the grid, the order inside a cell and wave timing.  The search bins the
 * train records into a uniform grid over the train context's W x H frame with cell(x) =
 * clamp(floorf(x * (1 / c)), 0, G - 1), c a power of two: monotone in x, so the cells cell(x0) ..
 * cell(x1) hold every candidate whatever the arithmetic rounds.  Out of scope: a circular window, the
 * mutual test, a fit that reads this list on the device (gdp_ransac_set_input takes it). */
typedef struct gdp_guided gdp_guided;
/* A guided-matching object reading one fit object (non-NULL) and, through it, the match object and its
 * two describe objects: all are only read — looked up at every launch — and must outlive this object:
 * destroy this one first.  It owns an output buffer of the match object's query capacity (so it cannot
 * overflow), one uint32 counter, the grid arrays, its per-record scratch and the caller's matrix.
 * max_cells bounds the grid of a launch (0: 262,144; above 16,777,216 is GDP_ERR_ARG).
 * gdp_guided_last_error(g) describes g's last failure (g NULL: this thread's last failed create). */
int gdp_guided_create(gdp_guided** out, const gdp_ransac* src, uint32_t max_cells);
void gdp_guided_destroy(gdp_guided* g);
const char* gdp_guided_last_error(const gdp_guided* g);
/* Make h9[0..9) the model instead of the fit's model record (blocking).  The floats are not validated
 * (point 8 of the rule).  NULL goes back to the fit's model record. */
int gdp_guided_set_model(gdp_guided* g, const float* h9);
/* Match: zeroes the counter and the grid on `stream` (NULL = the QUERY context's own stream), then
 * launches; asynchronous and stream-ordered.  The two lists' counts and the model record are read on
 * the device, the host never reads them, so launching this right after gdp_fit_homography on the same
 * stream is the normal use.  `radius` must be finite and >= 0 and `ratio` 0 (no ratio test) or in
 * (0, 1]; a NaN, anything else or an image index out of range is GDP_ERR_ARG and nothing changes: the
 * previous result stays downloadable.  The device order is unspecified. */
int gdp_match_guided(gdp_guided* g, int query_image, int train_image, float radius, float ratio, uint32_t max_distance,
                     int unique, void* stream);
/* Records the last launch produced (blocking; waits for the query context's OWN stream; 0 before any). */
int gdp_guided_count(gdp_guided* g, size_t* found);
/* Copy min(found, `capacity`) records to `host` (blocking), sorted ascending by `query`, which is
 * unique per record.  *stored = records written, *found = gdp_guided_count (either may be NULL). */
int gdp_download_guided(gdp_guided* g, gdp_match_record* host, size_t capacity, size_t* stored, size_t* found);
/* Zero-copy view for device consumers: the records (the match object's query capacity of them, the
 * first *count valid, device order) and the counter. */
int gdp_device_guided(const gdp_guided* g, const gdp_match_record** records, const uint32_t** count);
/* The grid of the LAST launch (any output may be NULL): the cell side c — the smallest power of two >=
 * max(radius / 2, 1), doubled until the train frame takes at most max_cells cells — and the cells per row
 * and per column, ceil(W / c) x ceil(H / c) (0 and 0 x 0 before any launch); the object's max_cells;
 * and the lanes that share one query in the search. */
int gdp_guided_layout(const gdp_guided* g, float* cell_side, uint32_t* cells_x, uint32_t* cells_y, uint32_t* max_cells,
                      uint32_t* lanes_per_query);

/* ---- output --------------------------------------------------------------------------------
 * The blocking copies below are ordered after work on the context's OWN stream; if a build was
 * launched on another stream, synchronize that stream first. */
/* Device pointer to level (o, s) of image b: rows x cols float32, row-major, dense.  The pointer
 * is const: read through it freely.  Whoever casts the const away and WRITES through it (a
 * collective receiving into the pyramid, a caller's own kernel) calls gdp_pyramid_written on this
 * context before its next gdp_build — libgdp tracks its own writers, not foreign ones, and a build
 * on a pyramid it believes untouched keeps the input-independent zeros an earlier build stored
 * (GDP_TUNE_KEEP_ZEROS). */
const float* gdp_device_level(const gdp_ctx* ctx, int b, int octave, int scale);
/* Tell the context that image b's pyramid (b < 0: every image's) was, or is about to be, written
 * by something other than libgdp: the next gdp_build stores every byte again.  Host-side flag
 * only (no device work, no synchronisation); order the write itself against the build as for any
 * two device operations. */
int gdp_pyramid_written(gdp_ctx* ctx, int b);
/* Copy level (o, s) of image b to a dense host array (blocking). */
int gdp_download_level(gdp_ctx* ctx, int b, int octave, int scale, float* host);
/* Copy level (o, s) of image b into host row pointers — materialises the reference's
 * float**** GaussPy[o][s] rows (GuassDePyramid.h:16) (blocking). */
int gdp_download_level_rows(gdp_ctx* ctx, int b, int octave, int scale, float* const* rows);
/* Mirror image b's whole pyramid into the reference's host layout GaussPy[o][s][row] (the
 * float**** of GuassDePyramid.h:16; rows as held by this context), staging the levels through a
 * double-buffered pinned buffer (the D2H copy of one 32 MiB batch overlaps the host scatter of the
 * previous one; GDP_TUNE_STAGE_KB / _THREADS) (blocking).  What the drop-in classes call after
 * each mutating method. */
int gdp_download_pyramid_rows(gdp_ctx* ctx, int b, float* const* const* const* gauss_py);
/* Copy rows [first_row, first_row + nrows) of level (o, s) of image b (rows as held by this
 * context; a band context's row 0 is its first row) to a dense host array (blocking).  Reads one
 * GaussPy[o][s][r] row range without materialising the level (e.g. 65536^2 images). */
int gdp_download_level_range(gdp_ctx* ctx, int b, int octave, int scale, int first_row, int nrows, float* host);
/* Copy the whole pyramid of image b in the packed layout [o][s][rows][cols] (blocking). */
int gdp_download_pyramid(gdp_ctx* ctx, int b, float* host);
/* Upload a packed pyramid of image b (state restore; used by re-entry tests). */
int gdp_upload_pyramid(gdp_ctx* ctx, int b, const float* host);
/* Host -> device state: the reference's float**** GaussPy IS its pyramid, and GaussFilter /
 * GenerateDoG work on whatever the caller left in it (GuassDePyramid.h:16, :122-131, :140-146).
 * These copy a caller-edited host pyramid back into the device levels (blocking), so an in-place
 * call that follows processes the caller's edits.  The drop-in classes call them before every
 * mutating method when `mirror_host` is set or the caller flagged `host_dirty`
 * (include/GaussDePyramid-HIP.h).
 *   gdp_upload_level:        level (o, s) of image b from a dense rows x cols host array
 *   gdp_upload_level_rows:   the same from host row pointers (GaussPy[o][s])
 *   gdp_upload_pyramid_rows: every level of image b from GaussPy[o][s][row] (the inverse of
 *                            gdp_download_pyramid_rows; rows gathered through the double-buffered
 *                            pinned staging, the H2D copy of one batch overlapping the gather of
 *                            the next)
 *   gdp_upload_image_raw:    image b's pyramid in the device layout (gdp_image_floats floats,
 *                            level (o, s) at gdp_level_offset(ctx, 0, o, s)) in ONE H2D copy — the
 *                            inverse of gdp_download_image_raw */
int gdp_upload_level(gdp_ctx* ctx, int b, int octave, int scale, const float* host);
int gdp_upload_level_rows(gdp_ctx* ctx, int b, int octave, int scale, const float* const* rows);
int gdp_upload_pyramid_rows(gdp_ctx* ctx, int b, const float* const* const* const* gauss_py);
int gdp_upload_image_raw(gdp_ctx* ctx, int b, const float* host);
/* Float elements of one image's packed pyramid (what gdp_download_pyramid writes). */
size_t gdp_packed_floats(const gdp_ctx* ctx);
/* Zero-copy output: write the pyramids into caller-owned DEVICE memory of at least
 * gdp_pyramid_bytes() bytes, 256-B aligned (e.g. a torch tensor that a collective then moves).
 * Level (o, s) of image b starts gdp_level_offset() floats into it.  base = NULL restores the
 * context's own buffer. */
int gdp_set_output_device(gdp_ctx* ctx, float* base, size_t bytes);
size_t gdp_level_offset(const gdp_ctx* ctx, int b, int octave, int scale);

/* ---- host mirror in the device layout (the drop-in classes' fast path) ---------------------
 * gdp_host_alloc: pinned (page-locked) host memory, which one DMA copy fills at the full PCIe
 * rate (gdp_host_free releases it).  gdp_image_floats: floats of one image's pyramid in the device
 * layout — level (o, s) at gdp_level_offset(ctx, 0, o, s), dense rows of cols_o floats, levels
 * 256-B aligned (the dense extent, also under a spread layout).  gdp_download_image_raw: copy
 * image b's pyramid in that layout to `host` in ONE
 * D2H copy (blocking).  A caller that points the reference's float**** rows into such a buffer
 * (GaussPy[o][s][r] = host + gdp_level_offset(ctx, 0, o, s) + r * cols_o) mirrors the device with
 * no per-row scatter (include/GaussDePyramid-HIP.h does). */
int gdp_host_alloc(size_t bytes, void** host);
void gdp_host_free(void* host);
size_t gdp_image_floats(const gdp_ctx* ctx);
int gdp_download_image_raw(gdp_ctx* ctx, int b, float* host);
/* GenerateDoG (in place, all octaves, the context's window centre) of image `b` held in HOST
 * memory in the raw device layout (gdp_download_image_raw's format, `gdp_image_floats` floats):
 * bit-identical to gdp_upload_image_raw(b, host) + gdp_generate_dog + gdp_download_image_raw(b,
 * host) for that image, but pipelined over row chunks so the host-to-device copies, the kernel and
 * the device-to-host copies overlap (two copy streams beside the context's).  `host` should be
 * pinned (gdp_host_alloc) for the copies to be asynchronous.  Blocking.  The overlap is
 * best-effort: the two copy streams share the process's hardware queues (4 on the MI355X boxes)
 * with every other stream and context, so under concurrent work the copies may serialise with
 * the kernel — the result is the same either way.  This is what the C++ drop-ins run for
 * GenerateDoG() when GaussPy is mirrored (mirror_host, the default) and not write-tracked. */
int gdp_generate_dog_mirrored(gdp_ctx* ctx, int b, float* host);

/* ---- write-tracked host mirrors (GuassDePyramid.h:16's two-way GaussPy, main.cpp:66-73) ------
 * A mirror that the caller usually does not write (main.cpp's loop never writes GaussPy) need not
 * be uploaded before every call.  gdp_host_alloc_tracked: `bytes` of host memory for such a mirror
 * — one shared-memory object mapped twice, a view registered with HIP that libgdp's copies use
 * (gdp_upload_image_raw / gdp_download_image_raw / gdp_generate_dog_mirrored* and the single-buffer
 * level / pyramid copies given an address inside it DMA through it at the pinned rate) and the returned CPU view, which is the one ever
 * write-protected (protecting memory the GPU driver registered — hipHostMalloc / hipHostRegister —
 * invalidates the registration and stalls the process's GPU queues, so gdp_host_track refuses such
 * memory).  Freed by gdp_host_free.  GDP_ERR_STATE / _HIP / _NOMEM: not available (use
 * gdp_host_alloc and whole uploads).  It is tracked from the start, not armed.
 * gdp_host_track registers other, plain (unregistered, page-granular) host memory and re-enables
 * tracking of an untracked gdp_host_alloc_tracked buffer; the first call installs a SIGSEGV
 * handler (once per process; faults elsewhere go to the handler installed before it, or take the
 * default action).  gdp_host_arm write-protects the buffer's pages — the caller asserts that the
 * buffer now equals the device copy it mirrors; the first CPU write to each page then faults once,
 * is recorded, and the page is writable again.  gdp_upload_image_written /
 * gdp_generate_dog_mirrored_written are gdp_upload_image_raw / gdp_generate_dog_mirrored that
 * upload only the pages written since the buffer was armed (the caller asserts image b's device
 * pyramid equals the buffer as of arming), and re-arm it; on a buffer that is not tracked or not
 * armed they upload everything (and arm it if tracked).  gdp_host_written_bytes: bytes of the
 * buffer in pages written since arming (GDP_ERR_STATE when not armed).  gdp_host_untrack makes
 * every page writable and stops recording (a gdp_host_alloc_tracked buffer keeps its DMA view).
 * Not seen (untrack such buffers): writes that do not fault on the CPU view — DMA into it, or a
 * system call such as read(2), which fails with EFAULT on a protected page.  GDP_ERR_STATE from
 * gdp_host_track: page protection is unavailable for this memory, it is registered with the GPU,
 * or no slot is free (64). */
int gdp_host_alloc_tracked(size_t bytes, void** host);
int gdp_host_track(void* host, size_t bytes);
int gdp_host_untrack(void* host);
int gdp_host_arm(void* host);
int gdp_host_written_bytes(const void* host, size_t* bytes);
int gdp_upload_image_written(gdp_ctx* ctx, int b, const float* host);
int gdp_generate_dog_mirrored_written(gdp_ctx* ctx, int b, float* host);
/* Deferred download (opt-in; the drop-in's GaussPyramid_hip::DeferDownload).  gdp_host_defer: the
 * caller asserts that image b's device pyramid of `ctx` is now NEWER than the tracked
 * gdp_host_alloc_tracked buffer `host` (at most gdp_image_floats floats), instead of downloading
 * it: every page of the CPU view becomes inaccessible, and the first CPU access to one (read or
 * write) faults, has a block of pages around it copied from the device — 64 pages, doubling to 8192
 * while the faults walk forward, then the next block ahead of the reader too (its first page stays
 * inaccessible until touched, which queues the one after) — on the context's stream by a libgdp
 * helper thread, and arms them
 * (a write then faults once more and is recorded, as above).  Not blocking: the fetches are ordered
 * after the work queued on the context's stream.  Host writes not uploaded yet are discarded (the
 * device copy is declared the newer one).  gdp_host_fetch completes a deferred buffer now (every
 * inaccessible page fetched; gdp_download_image_raw(b, host) of the whole image ends the deferral
 * by overwriting it).  Every libgdp entry taking caller host memory completes deferred buffers
 * first, and gdp_destroy completes those deferred to its context; gdp_host_untrack / gdp_host_arm
 * of a deferred buffer complete it first.  gdp_host_deferred_stats: bytes not fetched yet (whole
 * pages) and the bytes / copies fetched since the last gdp_host_defer (any argument may be NULL).
 * Limits on top of write tracking's: a system call READING a deferred page (write(2), send(2) from
 * it) fails with EFAULT, and a fault while the faulting thread holds a HIP runtime lock (the
 * buffer's CPU view handed straight to a HIP copy) cannot be served — call gdp_host_fetch before
 * either.  GDP_ERR_STATE: `host` is not a tracked gdp_host_alloc_tracked buffer. */
int gdp_host_defer(gdp_ctx* ctx, int b, void* host);
int gdp_host_fetch(void* host);
int gdp_host_deferred_stats(const void* host, size_t* stale_bytes, size_t* fetched_bytes, uint64_t* fetches);
/* Order-independent 64-bit checksum of image b's pyramid (blocking): the sum, mod 2^64, over
 * every word of every level of splitmix64_fin(idx * 0x9E3779B97F4A7C15 + (o*64+s) *
 * 0xD1B54A32D192ED03 + float_bits), idx = global_row * cols + col.  Row-band checksums add up
 * to the whole image's, so multi-GPU runs are verified by gathering 8 bytes per rank. */
int gdp_checksum(gdp_ctx* ctx, int b, uint64_t* out);

/* ---- taps ---------------------------------------------------------------------------------- */
/* The column (axis = 0, from W) or row (axis = 1, from H) window of (o, s) the context uploaded,
 * copied to host (cols_o or rows-of-whole-image_o floats).  Lets tests pin the host taps against
 * the reference's own (tests/golden/taps.npz). */
int gdp_get_taps(gdp_ctx* ctx, int axis, int octave, int scale, float* host);

/* ---- window centre ------------------------------------------------------------------------
 * Where the 1-D window of octave o is centred.  GDP_CENTRE_SERIAL (default): c = (len_f - 1) / 2
 * with len_f the FLOAT axis length halved o times (GuassDePyramid.h:107-115, also
 * GaussPyramid_mpi::GaussFilter, GaussDePyramid-MPI.h:134-143).  GDP_CENTRE_INTLEN:
 * c = float(len_o - 1) / 2 with the INTEGER length len_o = n >> o, what the multi-process variants
 * compute (GaussPyramid_mpi::GenerateDoG_mpi, GaussDePyramid-MPI.h:273; mpitest.cpp:44,123).  The
 * two agree bit for bit whenever every octave's float length is whole (n a multiple of
 * 2^(octaves-1)); they differ for e.g. n = 100 from octave 3 on.  Each mode has its own device
 * tap table, built and uploaded on its first use (a blocking copy); after that a switch only
 * selects the table the NEXT launch reads — no device drain, launches already queued keep the
 * table they were launched with.  Pure layout of the taps: kernels and bytes are unchanged. */
enum { GDP_CENTRE_SERIAL = 0, GDP_CENTRE_INTLEN = 1 };
int gdp_set_window_centre(gdp_ctx* ctx, int mode);
int gdp_get_window_centre(const gdp_ctx* ctx);

/* ---- band state ----------------------------------------------------------------------------
 * Copy the band's rows of every level of `full` (a whole-image context of the same H, W, S and
 * octaves) image `full_image` into band context `band` image `band_image`: the band then holds
 * exactly its rows of the whole pyramid's CURRENT contents, so an in-place call on the band
 * (gdp_generate_dog, gdp_gauss_octave, ...) continues where the whole image left off (the
 * operation is pointwise).  Device-to-device, ordered on `stream` (NULL = the band's stream),
 * blocking.  Before copying it waits for `full`'s OWN stream only: work the caller queued for
 * `full` on any other stream must be complete (or ordered before `stream`) when this is called.
 * (The C++ MPI drop-in does not use it: after single-process calls each rank re-enters on its
 * whole-image context instead, GaussDePyramid-HIP-mpi.h.) */
int gdp_copy_band(gdp_ctx* band, int band_image, const gdp_ctx* full, int full_image, void* stream);

/* ---- tuning (performance only; results are bit-identical for every setting) --------------- */
enum {
    GDP_TUNE_NONTEMPORAL = 1,   /* 1 (default): pyramid stores bypass cache allocation (nt)   */
    GDP_TUNE_BLOCKS_PER_CU = 2, /* value > 0: persistent build grid = CUs x value;
                                   0 (default): one 16x256 tile per block                      */
    GDP_TUNE_GRID = 3,          /* explicit build grid size; 0 (default) = automatic         */
    GDP_TUNE_VARIANT = 4,       /* build kernel code variant (block size / tile shape): one of
                                   the ids gdp_build_variants lists (others GDP_ERR_ARG); default
                                   chosen from the image width and the pyramid backing          */
    GDP_TUNE_TILE_ORDER = 5,    /* build tile order: 0 linear (default), 1 XCD-chunked,
                                   2 XCD row-interleaved                                       */
    GDP_TUNE_INPLACE_SUB = 6,   /* in-place DoG / re-entry passes: blocks per 1024-group chunk,
                                   1 / 2 / 4 / 8 / 16 (default 16 for one image, else 4 up to
                                   32 Mpix per launch, else 1); 0 = one level per wave (k_levels_x);
                                   -16 = 16 x 256 block tiles of k_build's shape (k_levels_tile) */
    GDP_TUNE_WINDOW_SUB = 7,    /* in-place window pass: blocks per chunk (4 default; 1, 2, 8, 16) */
    GDP_TUNE_CONV_KERNEL = 8,   /* gdp_build_gaussian: 0 register sweep (S <= 3), 1 LDS tiles,
                                   2 block tiles (default; one output row per wave, S <= 5) */
    GDP_TUNE_CONV_ROWS = 9,     /* gdp_build_gaussian: block tiles' rows per block (48 default;
                                   16 / 32 with 16 waves, 8 / 16 / 24 / 32 with 8); the sweep's
                                   rows per wave strip (16 / 32) */
    GDP_TUNE_CONV_ORDER = 11,   /* gdp_build_gaussian block order: bit 0 XCD-chunked, bit 1 odd
                                   sweep waves go bottom-up (sweep only), bit 2 octave o's block
                                   rows issued right after the octave-0 rows covering their input
                                   rows.  Default 5 (4 for one image of >= 2^27 pixels) */
    GDP_TUNE_BUILD_LDS = 12,    /* gdp_build: dynamic LDS bytes requested per block (0 default);
                                   used only to cap resident blocks per CU (occupancy) */
    GDP_TUNE_STAGE_KB = 13,     /* row-pointer downloads: KiB per half of the double-buffered
                                   pinned staging buffer (32768 default) */
    GDP_TUNE_STAGE_THREADS = 14, /* row-pointer downloads: host threads scattering a staged batch
                                   into the caller's rows (8 default, at most the host's threads) */
    GDP_TUNE_CONV_WAVES = 15,   /* gdp_build_gaussian block tiles: waves per block (16 default, 8) */
    GDP_TUNE_ZERO_WINDOW = 16,  /* 1 = 4-pixel groups outside the support of every window (all
                                   taps of their row or columns +0, any scale, either centre) skip
                                   their window loads: gdp_build stores their DoG levels as +0
                                   before the input lands and level S+2 as copysign(0, x); the
                                   in-place window passes (gdp_generate_dog, gdp_gauss_*) form
                                   v * 0.0f.  The same bits either way; 0 (default) off */
    GDP_TUNE_STORE_PACE = 17,   /* -1 (default) off; n = 0..3: after each pyramid store of the
                                   build (full, subset and outside-support paths), wait until at
                                   most n memory operations of the wave are outstanding
                                   (s_waitcnt vmcnt(n)); the same bits either way */
    GDP_TUNE_CONV_PACE = 18,    /* the same for gdp_build_gaussian's block tiles (default 2) */
    GDP_TUNE_INPLACE_PACE = 19, /* the same for the in-place re-entry (gdp_generate_dog, k_levels;
                                   default -1): its own field, so tuning the build's pacing never
                                   changes the in-place passes' speed */
    GDP_TUNE_PYRAMID_CHUNK_KB = 20, /* read-only: how the context-owned pyramid is backed — KiB per
                                      separately created physical piece (default 2 MiB, at most
                                      4096 pieces), -1 one piece per image, 0 one hipMalloc */
    GDP_TUNE_KEEP_ZEROS = 21,   /* 1 (default): a gdp_build into the context-owned pyramid that
                                   follows another one, with no pyramid writer in between, does not
                                   store the S+2 DoG levels outside the windows' support again —
                                   they are +0 for any input and already there; level S+2 and the
                                   support are stored as ever.  The same bits either way; 0 = every
                                   build stores every byte.  A launch-time flag: no drain */
    GDP_TUNE_ZEROS_CLEAN = 22,  /* read-only: 1 while the next gdp_build may skip those stores (set
                                   by a gdp_build into the context-owned pyramid, cleared by every
                                   call that writes, moves or rebinds pyramid memory and by
                                   gdp_pyramid_written) */
    GDP_TUNE_KEEP_SIGNS = 24,   /* 1 (default): a steady-state build by k_keep (GDP_TUNE_KEEP_KERNEL
                                   >= 1) on int32 input does not store level S+2 = copysign(0, x)
                                   again where it would store +0 over +0: the context keeps a sign
                                   map on the device, one byte per input row of a 16 x 256 tile,
                                   and a row with no negative pixel now and none at the build
                                   before stores nothing.  The first such build after anything that
                                   clears GDP_TUNE_ZEROS_CLEAN, or after any other kind of build,
                                   stores everything and writes the map; the saving starts with the
                                   second.  A build that skips by the map runs k_keep with 4 rows
                                   per wave above 4 Mpix (it barely stores; read-only
                                   GDP_TUNE_KEEP_SIGNS_KERNEL), unless GDP_TUNE_KEEP_KERNEL was set
                                   by the caller; the build that writes the map makes every store
                                   and keeps GDP_TUNE_KEEP_KERNEL's shape.  uint8 input stores as before.  The same bits
                                   either way; 0 = every steady-state build stores all of level
                                   S+2.  A launch-time flag: no drain */
    GDP_TUNE_SIGNS_KNOWN = 25,  /* read-only: 1 while the sign map describes the context's pyramid
                                   (set by an int32 k_keep build with GDP_TUNE_KEEP_SIGNS = 1,
                                   cleared by whatever clears GDP_TUNE_ZEROS_CLEAN, by every other
                                   build and by a switch of GDP_TUNE_KEEP_SIGNS) */
    GDP_TUNE_KEEP_SIGNS_KERNEL = 26, /* read-only: the k_keep shape (a GDP_TUNE_KEEP_KERNEL value) of a
                                   build that skips by the sign map; 0 while GDP_TUNE_KEEP_KERNEL is 0 */
    GDP_TUNE_KEEP_SUPPORT = 27, /* 1 (default): k_keep runs the 4-pixel groups of the tiles that meet
                                   the windows' support — the only ones that are computed, not just
                                   given their sign — as work units of their own, 256 groups each,
                                   dispatched ahead of the 16 x 256 tiles, instead of in several
                                   serial rounds at the end of those tiles' blocks.  0 = in the
                                   tiles' blocks.  Every word is stored by the same code from the
                                   same pixel: the same bits either way, and a switch leaves
                                   GDP_TUNE_ZEROS_CLEAN and GDP_TUNE_SIGNS_KNOWN as they are.  A
                                   launch-time flag: no drain */
    GDP_TUNE_KEEP_SUPPORT_UNITS = 28, /* read-only: the number of those units in the context's next
                                   k_keep launch; 0 with GDP_TUNE_KEEP_SUPPORT = 0 or where k_keep
                                   does not take the context (GDP_TUNE_KEEP_KERNEL) */
    GDP_TUNE_KEEP_KERNEL = 23  /* the kernel of a gdp_build that skips those stores (the steady
                                   state): 0 = the build kernel's own keep path; 1, 2 = the
                                   steady-state kernel k_keep — one pass over the input on
                                   16 x 256 tiles, level S+2 of every fused octave stored from the
                                   registers that hold the octave-0 pixels — with 4 or 2 rows per
                                   wave (default by pixels per launch: 0 under 1.5 Mpix, 2 up to 64 Mpix,
                                   1 above).  Taken when the width is a multiple of 4 and the input
                                   allows one vector load per 4 pixels; any other context runs 0.
                                   The same bits either way.  A launch-time flag: no drain */
};
int gdp_set_tuning(gdp_ctx* ctx, int key, int value);
/* The build-kernel variant ids this library holds (GDP_TUNE_VARIANT values): writes up to
 * `capacity` of them to `ids` (may be NULL) and returns how many there are.  Pure table read: no
 * device, no context. */
int gdp_build_variants(int* ids, int capacity);
/* Benchmark every build-kernel variant x tile order x store mode (GDP_TUNE_ZERO_WINDOW,
 * GDP_TUNE_STORE_PACE) in (0, off) (0, 1) (1, off) (1, 0) on the context's current input (`iters`
 * launches each, HIP events on `stream`) and keep the fastest; reports the variant, tile order
 * (the store mode: gdp_get_tuning) and its per-launch ms.  Results are bit-identical for every
 * candidate.  Overwrites the pyramid.  NB: GDP_TUNE_ZERO_WINDOW is context-wide — the pick also
 * applies to the in-place window passes that run later on this context (bit-identical either
 * way); GDP_TUNE_STORE_PACE applies to the builds only (the re-entry has GDP_TUNE_INPLACE_PACE). */
int gdp_autotune(gdp_ctx* ctx, int iters, void* stream, int* variant, int* tile_order, float* ms_per_build);
int gdp_get_tuning(const gdp_ctx* ctx, int key, int* value);

/* ---- misc ---------------------------------------------------------------------------------- */
int gdp_sync(gdp_ctx* ctx);                    /* wait for the context's stream */
void* gdp_stream(const gdp_ctx* ctx);          /* the context's own hipStream_t */
const char* gdp_last_error(const gdp_ctx* ctx); /* ctx may be NULL: last create() failure */
const char* gdp_status_string(int status);
/* Time `iters` back-to-back gdp_build launches on `stream` with HIP events recorded on that same
 * stream; writes the total milliseconds.  Used by bench.py for the per-launch kernel time.  Two
 * untimed builds run first, so every timed launch finds the pyramid in the same state (clean, with
 * GDP_TUNE_KEEP_ZEROS, after the first; the sign map known, with GDP_TUNE_KEEP_SIGNS, after the
 * second: the steady state of a context that is built again and again; the cost of a
 * first build is what GDP_TUNE_KEEP_ZEROS = 0 times).  gdp_autotune times its candidates this way. */
int gdp_time_builds(gdp_ctx* ctx, int iters, void* stream, float* total_ms);

#ifdef __cplusplus
}
#endif

#endif /* GDP_H_ */
