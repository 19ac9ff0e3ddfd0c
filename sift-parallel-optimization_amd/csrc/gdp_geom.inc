// gdp_geom.inc — Geometry structs (device-resident Geom), constants and the device load/store helpers.
// Part of libgdp's single translation unit: included by gdp.hip inside its anonymous namespace
// (after `#pragma clang fp contract(off)`, which therefore applies here too).  Not a header.

// ------------------------------------------------------------------------------------------
// geometry
// ------------------------------------------------------------------------------------------
constexpr int kMaxOct = 32;
constexpr int kBlock = 256;     // 4 waves (in-place / synthetic kernels)
constexpr int kTailGroups = 256; // groups of 4 pixels per tail work unit
constexpr int kLevBlock = 1024;  // threads (= 4-pixel groups) per block of the in-place passes
constexpr int kLtRows = 16;      // rows of the in-place block tiles (k_levels_tile, 16 x 256 like k_build's)
constexpr int kFused = 5;       // octaves 0..4 share one 16 x 256 input tile
constexpr int kTileRows = 16;   // 2^(kFused-1): every fused octave has whole rows in a tile
constexpr int kTileCols = 256;  // tile width of the register octave-0 path (64 lanes x 4 pixels)
constexpr int kLevelAlign = 64; // floats (256 B) — every level starts 16-B (and 256-B) aligned
constexpr size_t kStageFloats = size_t(16) << 20;  // pinned D2H staging chunk (64 MiB)

struct OctGeom {
    int rows;             // output rows of this octave held by the context (band-local)
    int row0;             // global output row of band-local row 0
    int cols;             // W >> o
    int gpr;              // groups of 4 columns per row, ceil(cols / 4)
    long long lev_off;    // floats from an image's pyramid base to level (o, 0)
    long long lev_stride; // floats from level (o, s) to (o, s+1)
    int ctap;             // float offset of column taps (o, 0) in the tap table
    int ctap_stride;      // floats between scales (multiple of 4, zero padded)
    int rtap;             // float offset of row taps (o, 0), indexed by GLOBAL output row:
    int rtap_stride;      //   tap (o, s) of row r at rtap + r * rtap_row + s * rtap_stride
    int rtap_row;         //   (square: the column taps, rtap_row 1; else [row][scale]: rtap_row L, stride 1)
    long long grp_begin;  // prefix (over octaves 0..o-1) of rows*gpr per image
    unsigned long long gpr_magic; // fast k / gpr for k < 2^31: (k * magic) >> gpr_shift
    int gpr_shift;
    // Window support (GDP_TUNE_ZERO_WINDOW): global rows [nz_r0, nz_r1) / columns [nz_c0, nz_c1)
    // hold every non-zero row / column tap of this octave (any scale, either window centre).
    // Outside them every tap of a pixel's row or column is +0, so G_s = (x * fc) * fr is a zero
    // with x's sign for every s: the DoG levels are +0 for any input and level S+2 is
    // copysign(0, x).  With the knob off the ranges cover the whole octave.
    int nz_r0, nz_r1, nz_c0, nz_c1;
    // The in-place passes' row range: (v * fc) * fr == v * 0.0f for a row outside the support
    // (fr = +0) only when v * fc cannot overflow to inf (inf * 0 = NaN), i.e. when every column tap
    // of the octave is <= 1 — true for S <= 2 (peak tap (s+1) / (2 sqrt(2 PI)) > 1 from s = 5 on).
    // The build's int32 inputs never overflow (|x| < 2^31, taps < 2), so it uses nz_r*; the in-place
    // passes use these, which cover the whole octave when some column tap exceeds 1 (ADVICE r3).
    int nzi_r0, nzi_r1;
    // The TRUE window support, whatever the knob says (set once at context creation, both window
    // centres): the build's `keep` test (outside_support).  On a clean pyramid the DoG levels of a
    // group outside these ranges already hold their +0, so the build does not store them again.
    int sp_r0, sp_r1, sp_c0, sp_c1;
    int span;            // contiguous-span build variants (PATH 4): groups of this octave per unit
};

// Group (global row Rg, columns C..C+n-1) outside the support of every window of its octave
// (GDP_TUNE_ZERO_WINDOW; always false with the knob off, the ranges then cover the octave).
__device__ __forceinline__ bool zero_support(const OctGeom& og, int Rg, int C, int n) {
    return Rg < og.nz_r0 || Rg >= og.nz_r1 || C + n <= og.nz_c0 || C >= og.nz_c1;
}

// Group outside the true support (OctGeom::sp_*, independent of GDP_TUNE_ZERO_WINDOW): its DoG
// levels are +0 for any input — the stores a build skips on a clean pyramid (k_build's `keep`).
__device__ __forceinline__ bool outside_support(const OctGeom& og, int Rg, int C, int n) {
    return Rg < og.sp_r0 || Rg >= og.sp_r1 || C + n <= og.sp_c0 || C >= og.sp_c1;
}

// The same for the in-place window passes on caller-written floats (OctGeom::nzi_*): a column
// outside the support (fc = +0) gives (v * 0) * fr == v * 0.0f for every v; a row outside it only
// where no column tap exceeds 1.
__device__ __forceinline__ bool zero_support_ip(const OctGeom& og, int Rg, int C, int n) {
    return Rg < og.nzi_r0 || Rg >= og.nzi_r1 || C + n <= og.nz_c0 || C >= og.nz_c1;
}

// GDP_TUNE_STORE_PACE: after a pyramid store, wait until at most n vector-memory operations of
// this wave are outstanding (s_waitcnt vmcnt(n); expcnt / lgkmcnt left at their maxima), so a wave
// keeps about n + 1 stores in flight — the pacing the full build's window loads give its stores
// (gfx9's in-order vmcnt).  n < 0: no wait.  n is wave-uniform (a scalar branch).
__device__ __forceinline__ void pace_stores(int n) {
    switch (n) {
        case 0: __builtin_amdgcn_s_waitcnt(0x0F70); break;
        case 1: __builtin_amdgcn_s_waitcnt(0x0F71); break;
        case 2: __builtin_amdgcn_s_waitcnt(0x0F72); break;
        case 3: __builtin_amdgcn_s_waitcnt(0x0F73); break;
        default: break;
    }
}

// A store pace template argument meaning "the run-time value" (compile-time paces are >= -1).
constexpr int kPaceRuntime = -2;

// Granlund-Montgomery division by an invariant d >= 1 for numerators n < 2^31:
// magic = ceil(2^(31+l) / d), l = ceil(log2 d); n / d == (n * magic) >> (31 + l).
inline void make_magic(unsigned d, unsigned long long* magic, int* shift) {
    int l = 0;
    while ((1ull << l) < d) ++l;
    *shift = 31 + l;
    *magic = ((1ull << *shift) + d - 1) / d;
}

__device__ __forceinline__ unsigned fast_div(unsigned n, unsigned long long magic, int shift) {
    return (unsigned)(((unsigned long long)n * magic) >> shift);
}

struct Geom {
    int H, W, S, L, O, F, batch;
    int in_rows, in_row0; // input rows held (band) and their first global row
    int vec_in;           // one vector load per 4 pixels legal (pitch % 4 == 0, base aligned)
    int tile_order;       // GDP_TUNE_TILE_ORDER
    int in_fmt;           // GDP_INPUT_I32 / GDP_INPUT_U8
    int store_pace;       // GDP_TUNE_STORE_PACE: < 0 off, else vmcnt bound after each pyramid store
    int conv_pace;        // GDP_TUNE_CONV_PACE: the same for the convolution block tiles (default 2)
    int inplace_pace;     // GDP_TUNE_INPLACE_PACE: the same for the in-place re-entry (k_levels)
    long long in_pitch, in_img_stride;
    long long pyr_stride; // floats between image pyramids
    int tiles_r, tiles_c;
    unsigned tiles_per_img, tiles_total;       // host checks the unit count fits 31 bits
    unsigned tail_groups_per_img, tail_units;  // octaves >= F, 256 groups per unit
    int span_rest;        // contiguous-span variants: sum of OctGeom::span over octaves >= 1
    int pad_span_;
    // k_keep (gdp_keep.inc, GDP_TUNE_KEEP_KERNEL): its own kTileRows x kTileCols tile grid and tail
    // split (octaves >= kp_F), set once at context creation — independent of the selected build variant
    int kp_F, kp_tiles_c;
    int kp_row_start, kp_pad_; // first tile row that meets some fused octave's support: k_keep's tile order starts there
    unsigned kp_tiles_per_img, kp_tiles_total;
    unsigned kp_tail_groups_per_img, kp_tail_units;
    // k_keep's support units (GDP_TUNE_KEEP_SUPPORT), set with the support (set_window_support).  Per
    // fused octave o < kp_F the tiles whose footprint meets the support (OctGeom::sp_*) are the
    // rectangle of tile rows [kp_sl_tr0, kp_sl_tr1) x tile columns [kp_sl_tc0, kp_sl_tc1) (band-local
    // tile rows; empty: tr0 == tr1): the kernel classifies a (tile, octave) pair by these alone.  The
    // octave's footprint of that rectangle, clipped to the rows and columns the context holds, in
    // 4-pixel groups: kp_sg_rows rows from band-local octave row kp_sg_r0, kp_sg_gpr groups per row
    // from column kp_sg_c0.  kp_sup_begin: prefix over the fused octaves of rows * gpr per image;
    // kp_sup_units: 256-group slices of [batch][kp_sup_begin[kp_F]].
    int kp_sl_tr0[kFused], kp_sl_tr1[kFused], kp_sl_tc0[kFused], kp_sl_tc1[kFused];
    int kp_sg_r0[kFused], kp_sg_rows[kFused], kp_sg_c0[kFused], kp_sg_gpr[kFused];
    unsigned kp_sup_begin[kFused + 1];
    unsigned kp_sup_units, kp_sup_pad_;
    OctGeom oct[kMaxOct];
    unsigned lv_blk[kMaxOct + 1]; // prefix over octaves of ceil(rows*gpr / kLevBlock) per image
    unsigned lx_blk[kMaxOct + 1]; // prefix over octaves of ceil(rows*gpr / 64) per image (k_levels_x)
    unsigned lt_blk[kMaxOct + 1]; // prefix over octaves of kLtRows x 256-column tiles per image (k_levels_tile)
    unsigned cv_blk[kMaxOct + 1]; // convolution mode: prefix over octaves of 16x256 output tiles
    int cv_tiles_c[kMaxOct];      // convolution mode: tile columns per octave
    unsigned sw_blk[kMaxOct + 1]; // convolution sweep: prefix over octaves of blocks (4 strips of T rows);
                                  // octaves whose width is not a multiple of 4 count 0 (tiles do them)
    int sw_strips_c[kMaxOct];     // convolution sweep: 240-column strips per octave
    unsigned cvx_blk[kMaxOct + 1]; // convolution tiles for the octaves the sweep skips
    // convolution extension on a row band: input rows above [0] / below [1] the band (halo rows,
    // gdp_conv_halo_rows), read from these device buffers [batch][halo_rows][halo_pitch]
    const void* halo_ptr[2];
    long long halo_pitch[2], halo_img_stride[2];
    int halo_rows[2];
    unsigned bk_blk[kMaxOct + 1];  // convolution block tiles (k_conv_blk): prefix over octaves of
                                   // T-row x 240-column tiles (same octaves as the sweep)
    int bk_strips_c[kMaxOct];      // convolution block tiles: tile columns per octave
    unsigned ex_blk[kMaxOct + 1];  // extrema detection (k_extrema): prefix over octaves of wave units,
                                   // kExRows candidate rows x kExStrip groups (0 for octaves under 3 x 3)
    int ex_strips[kMaxOct];        // extrema detection: strips per octave
};

typedef float f4 __attribute__((ext_vector_type(4)));
typedef int i4 __attribute__((ext_vector_type(4)));

// ------------------------------------------------------------------------------------------
// device helpers
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ f4 ld_f4(const float* p) { return *reinterpret_cast<const f4*>(p); }

// Streaming load of pyramid data that is read once per pass (in-place passes): non-temporal.
template <bool NT>
__device__ __forceinline__ f4 ld_stream(const float* p) {
    if constexpr (NT)
        return __builtin_nontemporal_load(reinterpret_cast<const f4*>(p));
    else
        return *reinterpret_cast<const f4*>(p);
}

template <bool NT>
__device__ __forceinline__ void st_f4(float* p, f4 v) {
#ifdef GDP_STORE_POLICY
    // timing-only builds (tools/ab): the streaming stores with another cache policy, e.g.
    // -DGDP_STORE_POLICY='"sc0 sc1"' (write-through, the line is not kept in L2)
    // NOT bit-exact on gfx950: the compiler does not treat the asm's data VGPRs as in flight
    // and may overwrite them before the store reads them (profiles/wt_check_r02am.log)
    if constexpr (NT) {
        asm volatile("global_store_dwordx4 %0, %1, off " GDP_STORE_POLICY : : "v"(p), "v"(v) : "memory");
        return;
    }
#endif
    if constexpr (NT)
        __builtin_nontemporal_store(v, reinterpret_cast<f4*>(p));
    else
        *reinterpret_cast<f4*>(p) = v;
}

// Stores the first `n` lanes of v (n in 1..4) — ragged right edge or unaligned rows.
__device__ __forceinline__ void st_part(float* p, f4 v, int n, bool aligned_full) {
    if (aligned_full) {
        *reinterpret_cast<f4*>(p) = v;
        return;
    }
    p[0] = v.x;
    if (n > 1) p[1] = v.y;
    if (n > 2) p[2] = v.z;
    if (n > 3) p[3] = v.w;
}

// Input pixels (R, C..C+3) of octave o for image b as float (zero beyond the row end).  The
// input is int32 (the reference's `int** img`) or uint8 (GDP_INPUT_U8: 4x fewer input bytes);
// the format is a wave-uniform scalar branch.  (float) of an int32 or uint8 value is the same
// single rounding the reference's `GaussPy[..] = data[..]` assignment performs (:80).
__device__ __forceinline__ f4 load_px(const Geom* __restrict__ g, const void* __restrict__ in, int b, int o,
                                      int Rg, int C, int n) {
    const long long in_row = ((long long)Rg << o) - g->in_row0;
    const long long row_off = (long long)b * g->in_img_stride + in_row * g->in_pitch;
    f4 x = {0.f, 0.f, 0.f, 0.f};
    if (g->in_fmt == GDP_INPUT_U8) {
        const unsigned char* row = static_cast<const unsigned char*>(in) + row_off;
        if (o == 0 && n == 4 && g->vec_in) {
            const unsigned w = *reinterpret_cast<const unsigned*>(row + C);
            x.x = (float)(w & 0xffu);
            x.y = (float)((w >> 8) & 0xffu);
            x.z = (float)((w >> 16) & 0xffu);
            x.w = (float)(w >> 24);
            return x;
        }
        x.x = (float)row[(long long)C << o];
        if (n > 1) x.y = (float)row[(long long)(C + 1) << o];
        if (n > 2) x.z = (float)row[(long long)(C + 2) << o];
        if (n > 3) x.w = (float)row[(long long)(C + 3) << o];
        return x;
    }
    const int* row = static_cast<const int*>(in) + row_off;
    if (o == 0 && n == 4 && g->vec_in) {
        const i4 v = *reinterpret_cast<const i4*>(row + C);
        return __builtin_convertvector(v, f4);
    }
    x.x = (float)row[(long long)C << o];
    if (n > 1) x.y = (float)row[(long long)(C + 1) << o];
    if (n > 2) x.z = (float)row[(long long)(C + 2) << o];
    if (n > 3) x.w = (float)row[(long long)(C + 3) << o];
    return x;
}
