// gdp_keep.inc — k_keep: the steady-state build (GDP_TUNE_KEEP_KERNEL), a kernel of its own for a
// build on a clean context-owned pyramid (gdp_ctx::zeros_clean, k_build's `keep` = 1).
// Part of libgdp's single translation unit: included by gdp.hip inside its anonymous namespace
// (after `#pragma clang fp contract(off)`, which therefore applies here too).  Not a header.
//
// On a clean pyramid the only bytes a build owes outside the windows' support are level S+2 =
// copysign(0, x): the sign bit of the input pixel.  Level S+2 of octave o at (r, c) is the sign of
// input pixel (r << o, c << o), so the lane that loaded that pixel for octave 0 stores it for every
// fused octave too: one pass over the input, every load of a lane issued before its first store,
// no second (decimated, strided) read of the input, no LDS, no cross-lane move, no conversion.
// k_build's keep path does the same work one 4-pixel group per thread, reading the input again for
// octaves 1-4 (DESIGN §10); it stays as the fallback (contexts this kernel does not take) and as
// GDP_TUNE_KEEP_KERNEL = 0.
//
// The sign map (GDP_TUNE_KEEP_SIGNS, gdp_ctx::d_signs): pixel intensities are non-negative, so on
// real input every one of those stores writes +0 over the +0 the build before left there.  The
// context keeps one byte per (image, tile, tile row) — [batch][kp_tiles_per_img][kTileRows] — that
// only this kernel's int32 register stores maintain.  While the host holds the map valid
// (gdp_ctx::signs_known), byte = 0 means: every level-S+2 word keep_tile_fast stores from that
// input row within the tile's 256 columns holds +0 in the context's pyramid, in every fused octave
// (octave o stores from rows = 0 mod 2^o only; the set of fast (tile, octave) pairs is fixed per
// context, OctGeom::sp_*).  A row whose byte is 0 and whose 256 pixels are all non-negative owes
// no store at all.  `signs`: kSignsOff — store everything, never touch the map; kSignsEstablish —
// store everything and write every row's byte; kSignsUse — skip such rows, keep the bytes current.
enum { kSignsOff = 0, kSignsEstablish = 1, kSignsUse = 2 };

typedef float f2 __attribute__((ext_vector_type(2)));

template <bool NT>
__device__ __forceinline__ void st_f2(float* p, f2 v) {
    if constexpr (NT)
        __builtin_nontemporal_store(v, reinterpret_cast<f2*>(p));
    else
        *reinterpret_cast<f2*>(p) = v;
}

template <bool NT>
__device__ __forceinline__ void st_f1(float* p, float v) {
    if constexpr (NT)
        __builtin_nontemporal_store(v, p);
    else
        *p = v;
}

// Tail unit `tu` of the octaves >= Geom::kp_F: build_tail_unit's walk on k_keep's own split (the
// selected build variant's F and tail counts differ), every group through build_group's keep path.
template <bool NT, int BLK>
__device__ __forceinline__ void keep_tail_unit(const Geom* __restrict__ g, const void* __restrict__ in,
                                               float* __restrict__ out, const float* __restrict__ taps, unsigned tu) {
    const int F = g->kp_F;
    for (int q = threadIdx.x; q < kTailGroups; q += BLK) {
        const unsigned t = tu * kTailGroups + q;
        const unsigned per = g->kp_tail_groups_per_img;
        if (t >= per * (unsigned)g->batch) break;
        const unsigned b = t / per;
        const long long rem = (long long)(t - b * per) + g->oct[F].grp_begin;
        int o = F;
        while (o + 1 < g->O && rem >= g->oct[o + 1].grp_begin) ++o;
        const OctGeom og = g->oct[o];
        const int k = (int)(rem - og.grp_begin);
        const int Rl = k / og.gpr;
        const int C = 4 * (k - Rl * og.gpr);
        build_group<0, NT, false>(g, in, out, taps, 1, (int)b, o, og, Rl, C);
    }
}

// Support unit `su` (GDP_TUNE_KEEP_SUPPORT): 256 consecutive groups of the fused octaves' support
// rectangles (Geom::kp_sg_*: the groups of every (tile, octave) pair whose footprint meets the
// support), flattened per image over the batch — the tail units' walk on another prefix, one group
// per thread on either block shape, every group through build_group's keep path as in the tile's
// own block before.
template <bool NT>
__device__ __forceinline__ void keep_support_unit(const Geom* __restrict__ g, const void* __restrict__ in,
                                                  float* __restrict__ out, const float* __restrict__ taps, unsigned su) {
    if (threadIdx.x >= kTailGroups) return;
    const int F = g->kp_F;
    const unsigned t = su * kTailGroups + threadIdx.x;
    const unsigned per = g->kp_sup_begin[F];
    if (t >= per * (unsigned)g->batch) return;
    const unsigned b = t / per;
    const unsigned rem = t - b * per;
    int o = 0;
    while (o + 1 < F && rem >= g->kp_sup_begin[o + 1]) ++o;
    const OctGeom og = g->oct[o];
    const int k = (int)(rem - g->kp_sup_begin[o]);
    const int gpr = g->kp_sg_gpr[o];
    const int r = k / gpr;
    const int Rl = g->kp_sg_r0[o] + r;
    const int C = g->kp_sg_c0[o] + 4 * (k - r * gpr);
    build_group<0, NT, false>(g, in, out, taps, 1, (int)b, o, og, Rl, C);
}

// The register stores of one tile: wave w owns tile rows w RPL .. w RPL + RPL - 1, lane l columns
// 4 l .. 4 l + 3 of each.  Every load of the lane is issued before its first store (RPL KiB in
// flight per wave); a row or column beyond the image is clamped for the load (always in bounds, no
// divergent load) and masked for the stores.  I32 = false (uint8 input): a pixel has no sign, so
// level S+2 is +0 and nothing is read.  `fast` bit o: store octave o; row[o] / cols[o] / off[o]:
// rows held, columns and float offset of level (o, S+2) in the image's pyramid (0 rows beyond O).
// `flags`: the tile's kTileRows bytes of the sign map (I32 and signs != kSignsOff only).  A row's
// byte is the wave-wide OR of the sign bits of the 256 pixels the wave loaded for it (lanes clamped
// for the load hold copies of valid pixels of the same tile row or column range: harmless); the
// wave's RPL bytes are contiguous and RPL-aligned, read with one load issued with the pixels'.
// Every branch on them is wave-uniform.  A byte is written by lane 0 alone, never for a row beyond
// the image, and under kSignsUse only when it changes.  Establishing, the stores run first, each
// row's as soon as its pixels are there, and the flags are written after them.  Using the map, all
// rows' decisions are taken before the first store: a wave none of whose rows owes a store ends
// there, one whose rows all do runs the same straight-line stores as without the map.  SIGNS = false (kSignsOff, and uint8 input) compiles
// none of this: the kernel as it was before the map, at its speed.
template <bool NT, int RPL, bool I32, bool SIGNS>
__device__ __forceinline__ void keep_tile_fast(const Geom* __restrict__ g, const void* __restrict__ in,
                                               float* __restrict__ img_out, unsigned b, int in_r0, int in_c0, unsigned fast,
                                               const int (&rows)[kFused], const int (&cols)[kFused],
                                               const long long (&off)[kFused], unsigned char* flags, int signs) {
    static_assert(RPL == 2 || RPL == 4, "one aligned load of a wave's flags");
    static_assert(I32 || !SIGNS, "uint8 input has no sign: it never uses the map");
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = in_c0 + 4 * lane;
    const int rt0 = wave * RPL;  // first tile row of this wave
    const int in_rows = g->in_rows, W = g->W;
    const bool col_ok = c < W;
    i4 x[RPL];
    unsigned old = 0;  // byte j: the flag of row rt0 + j as the build before left it
    if constexpr (I32) {
        if constexpr (SIGNS) {
            if (signs == kSignsUse) {
                if constexpr (RPL == 4)
                    old = *reinterpret_cast<const unsigned*>(flags + rt0);
                else
                    old = *reinterpret_cast<const unsigned short*>(flags + rt0);
                old = (unsigned)__builtin_amdgcn_readfirstlane((int)old);
            }
        }
        const int* src = static_cast<const int*>(in) + (long long)b * g->in_img_stride + min(c, W - 4);
        const long long pitch = g->in_pitch;
#pragma unroll
        for (int j = 0; j < RPL; ++j)
            x[j] = *reinterpret_cast<const i4*>(src + (long long)min(in_r0 + rt0 + j, in_rows - 1) * pitch);
    } else {
#pragma unroll
        for (int j = 0; j < RPL; ++j) x[j] = i4{0, 0, 0, 0};
    }
    if constexpr (!SIGNS) {
        // the kernel as it was before the map, statement for statement (regrouped into the helper
        // below it ran uint8 input 2 % slower)
#pragma unroll
        for (int j = 0; j < RPL; ++j) {
            const int rr = in_r0 + rt0 + j;  // band-local input row
            const int rt = rt0 + j;          // row of the tile: rt % 2^o == 0 <=> rr % 2^o == 0 (in_r0 % 16 == 0)
            const f4 s = __builtin_bit_cast(f4, x[j] & (int)0x80000000u);
            if ((fast & 1u) && col_ok && rr < rows[0]) st_f4<NT>(img_out + off[0] + (long long)rr * cols[0] + c, s);
            if ((fast & 2u) && (rt & 1) == 0 && (rr >> 1) < rows[1] && (c >> 1) < cols[1])
                st_f2<NT>(img_out + off[1] + (long long)(rr >> 1) * cols[1] + (c >> 1), f2{s.x, s.z});
            if ((fast & 4u) && (rt & 3) == 0 && (rr >> 2) < rows[2] && (c >> 2) < cols[2])
                st_f1<NT>(img_out + off[2] + (long long)(rr >> 2) * cols[2] + (c >> 2), s.x);
            if ((fast & 8u) && (rt & 7) == 0 && (lane & 1) == 0 && (rr >> 3) < rows[3] && (c >> 3) < cols[3])
                st_f1<NT>(img_out + off[3] + (long long)(rr >> 3) * cols[3] + (c >> 3), s.x);
            if ((fast & 16u) && (rt & 15) == 0 && (lane & 3) == 0 && (rr >> 4) < rows[4] && (c >> 4) < cols[4])
                st_f1<NT>(img_out + off[4] + (long long)(rr >> 4) * cols[4] + (c >> 4), s.x);
        }
        return;
    }
    auto store_row = [&](int j) {
        const int rr = in_r0 + rt0 + j;
        const int rt = rt0 + j;
        const f4 s = __builtin_bit_cast(f4, x[j] & (int)0x80000000u);
        if ((fast & 1u) && col_ok && rr < rows[0]) st_f4<NT>(img_out + off[0] + (long long)rr * cols[0] + c, s);
        if ((fast & 2u) && (rt & 1) == 0 && (rr >> 1) < rows[1] && (c >> 1) < cols[1])
            st_f2<NT>(img_out + off[1] + (long long)(rr >> 1) * cols[1] + (c >> 1), f2{s.x, s.z});
        if ((fast & 4u) && (rt & 3) == 0 && (rr >> 2) < rows[2] && (c >> 2) < cols[2])
            st_f1<NT>(img_out + off[2] + (long long)(rr >> 2) * cols[2] + (c >> 2), s.x);
        if ((fast & 8u) && (rt & 7) == 0 && (lane & 1) == 0 && (rr >> 3) < rows[3] && (c >> 3) < cols[3])
            st_f1<NT>(img_out + off[3] + (long long)(rr >> 3) * cols[3] + (c >> 3), s.x);
        if ((fast & 16u) && (rt & 15) == 0 && (lane & 3) == 0 && (rr >> 4) < rows[4] && (c >> 4) < cols[4])
            st_f1<NT>(img_out + off[4] + (long long)(rr >> 4) * cols[4] + (c >> 4), s.x);
    };
    auto negative = [&](int j) -> unsigned {  // wave-uniform: some pixel of the row's 256 is negative
        return __ballot((x[j].x | x[j].y | x[j].z | x[j].w) < 0) != 0 ? 1u : 0u;
    };
    if (signs != kSignsUse) {
        // establishing: every store as ever, each row's as soon as its pixels are there; the flags after them
#pragma unroll
        for (int j = 0; j < RPL; ++j) store_row(j);
#pragma unroll
        for (int j = 0; j < RPL; ++j) {
            const unsigned neg = negative(j);
            if (lane == 0 && in_r0 + rt0 + j < in_rows) flags[rt0 + j] = (unsigned char)neg;
        }
        return;
    }
    // bit j of `run`: row rt0 + j runs its stores iff its flag is set (the build before left a -0
    // there) or a pixel of it is negative now
    constexpr unsigned kAll = (1u << RPL) - 1u;
    unsigned run = 0u;
#pragma unroll
    for (int j = 0; j < RPL; ++j) {
        const unsigned neg = negative(j);
        const unsigned was = (old >> (8 * j)) & 0xffu;
        if (was != neg && lane == 0 && in_r0 + rt0 + j < in_rows) flags[rt0 + j] = (unsigned char)neg;
        run |= ((was | neg) ? 1u : 0u) << j;
    }
    if (run == 0) return;  // +0 over +0 in every row of the wave: nothing owed
    if (run != kAll) {
#pragma unroll
        for (int j = 0; j < RPL; ++j)
            if (run >> j & 1u) store_row(j);
        return;
    }
#pragma unroll
    for (int j = 0; j < RPL; ++j) store_row(j);
}

// Work units: the support units (below) if any, then kp_tiles_total kTileRows x kTileCols input
// tiles, then kp_tail_units 256-group slices of the octaves >= kp_F — a grid of its own, whatever build
// variant is selected.  A block is kTileRows / RPL waves.  The host takes this kernel only when
// W % 4 == 0 and the input allows one vector load per 4 pixels, so every group is whole and every
// store aligned.  Per (tile, octave), wave-uniformly: the octave's footprint of the tile misses the
// support (OctGeom::sp_*; the host's tile rectangles Geom::kp_sl_*) -> the register stores above;
// else that octave's groups of the tile go through build_group's keep path, which tests each group
// and is exact by construction.  `support` != 0 (GDP_TUNE_KEEP_SUPPORT, a launch-time argument):
// those groups — at 4096^2 a central tile's 1364, three to six serial rounds of dependent loads and
// stores after the block's register pass — run as units of their own, [0, kp_sup_units) ahead of the
// tiles, one group per thread, and a tile's block does nothing for the octaves that meet the support.
// The same words from the same pixels by the same code either way.
template <bool NT, int RPL, bool SIGNS>
__global__ void __launch_bounds__(64 * kTileRows / RPL) k_keep(const Geom* __restrict__ g, const void* __restrict__ in,
                                                               float* __restrict__ out, const float* __restrict__ taps,
                                                               int support, unsigned char* sign_map, int signs) {
    constexpr int BLK = 64 * kTileRows / RPL;
    static_assert(kTileCols == 256 && kTileRows == 16 && kFused == 5 && kTileRows % RPL == 0, "k_keep's tile");
    static_assert(BLK >= kTailGroups, "a support unit is one group per thread");
    // Units: [0, sup_units) the support units — first, so they are dispatched first —, then the
    // tiles, then the tail units.  `support` = 0 (GDP_TUNE_KEEP_SUPPORT = 0), or no unit at all: the
    // groups inside the support stay in their tiles' blocks (below).
    const unsigned sup_units = support ? g->kp_sup_units : 0u;
    const unsigned tiles_end = sup_units + g->kp_tiles_total;
    const unsigned units = tiles_end + g->kp_tail_units;
    const int F = g->kp_F;
    for (unsigned u = blockIdx.x; u < units; u += gridDim.x) {
        if (u < sup_units) {
            keep_support_unit<NT>(g, in, out, taps, u);
            continue;
        }
        if (u >= tiles_end) {
            keep_tail_unit<NT, BLK>(g, in, out, taps, u - tiles_end);
            continue;
        }
        // Tile order.  With support units: plain linear.  Without: each image's tile rows in order,
        // but starting at the first row that meets the support (kp_row_start) and wrapping round — the
        // few tiles inside the support then take the per-group path below, chains of dependent loads
        // and stores several times a register tile's life, so they start early and run under the rest
        // of the launch instead of extending its end.  Any order gives the same bits.
        const unsigned ut = u - sup_units;
        const unsigned b = ut / g->kp_tiles_per_img;
        const unsigned rem = ut - b * g->kp_tiles_per_img;
        const unsigned kr = rem / (unsigned)g->kp_tiles_c;
        const unsigned tc = rem - kr * (unsigned)g->kp_tiles_c;
        const unsigned tiles_r = g->kp_tiles_per_img / (unsigned)g->kp_tiles_c;
        const unsigned row_start = sup_units ? 0u : (unsigned)g->kp_row_start;
        const unsigned tr = kr + row_start < tiles_r ? kr + row_start : kr + row_start - tiles_r;
        const int in_r0 = (int)tr * kTileRows; // band-local input row of the tile (in_row0 is a multiple of 16)
        const int in_c0 = (int)tc * kTileCols;
        // the octaves whose footprint of this tile lies outside the support: the tile is outside the
        // host's rectangle of tiles that meet it (Geom::kp_sl_*, the same intervals the support units
        // are cut from, so the two cannot disagree); and level S+2 of each (oct[o] beyond O is all
        // zero: no rows, nothing stored)
        unsigned fast = 0;
        int rows[kFused], cols[kFused];
        long long off[kFused];
#pragma unroll
        for (int o = 0; o < kFused; ++o) {
            const OctGeom& og = g->oct[o];
            const bool hit = (int)tr >= g->kp_sl_tr0[o] && (int)tr < g->kp_sl_tr1[o] && (int)tc >= g->kp_sl_tc0[o] &&
                             (int)tc < g->kp_sl_tc1[o];
            if (o < F && !hit) fast |= 1u << o;
            rows[o] = og.rows;
            cols[o] = og.cols;
            off[o] = og.lev_off + (long long)(g->L - 1) * og.lev_stride;
        }
        if (fast) {
            float* img_out = out + (long long)b * g->pyr_stride;
            // the tile's bytes of the sign map, by its position in the image (not by its place in the order)
            unsigned char* flags =
                sign_map + ((size_t)b * g->kp_tiles_per_img + tr * (unsigned)g->kp_tiles_c + tc) * (size_t)kTileRows;
            if (g->in_fmt == GDP_INPUT_U8)
                keep_tile_fast<NT, RPL, false, false>(g, in, img_out, b, in_r0, in_c0, fast, rows, cols, off, flags, kSignsOff);
            else
                keep_tile_fast<NT, RPL, true, SIGNS>(g, in, img_out, b, in_r0, in_c0, fast, rows, cols, off, flags, signs);
        }
        const unsigned slow = ~fast & ((1u << F) - 1u);
        if (!slow || sup_units) continue;  // with support units those groups are theirs
        // the groups of the other octaves, flattened over the block's threads (octave o of a tile is
        // (16 >> o) rows of (64 >> o) groups): as few rounds of build_group as the block allows
        int total = 0;
#pragma unroll
        for (int o = 0; o < kFused; ++o)
            if (slow >> o & 1u) total += (kTileRows >> o) * ((kTileCols / 4) >> o);
        for (int q = (int)threadIdx.x; q < total; q += BLK) {
            int o = 0, qq = q;
#pragma unroll
            for (int k = 0; k < kFused; ++k) {
                const int n = (slow >> k & 1u) ? (kTileRows >> k) * ((kTileCols / 4) >> k) : 0;
                if (o == k && qq >= n) {
                    qq -= n;
                    o = k + 1;
                }
            }
            const OctGeom og = g->oct[o];
            const int r = qq >> (6 - o), cg = qq & (((kTileCols / 4) >> o) - 1);
            const int Rl = (in_r0 >> o) + r, C = (in_c0 >> o) + 4 * cg;
            if (Rl < og.rows && C < og.cols) build_group<0, NT, false>(g, in, out, taps, 1, (int)b, o, og, Rl, C);
        }
    }
}

// GDP_TUNE_KEEP_KERNEL values >= 1: rows per lane (block = 16 / rows waves); all bit-identical.
struct KeepKernel {
    int id, block;
    void (*k[2][2])(const Geom*, const void*, float*, const float*, int, unsigned char*, int); // [uses the sign map][NT]
};
#define GDP_KEEP_KERNEL(ID, RPL)                                                      \
    KeepKernel {                                                                      \
        ID, 64 * kTileRows / RPL, {                                                   \
            {k_keep<false, RPL, false>, k_keep<true, RPL, false>}, {k_keep<false, RPL, true>, k_keep<true, RPL, true>} \
        }                                                                             \
    }
const KeepKernel kKeepKernels[] = {
    GDP_KEEP_KERNEL(1, 4), // 4 waves, 4 rows (4 KiB of loads) per wave
    GDP_KEEP_KERNEL(2, 2), // 8 waves, 2 rows per wave
    // (measured and dropped: 2 waves x 8 rows — 4096^2 0.050 vs 0.040 / 0.033 ms for 4 / 2 rows, behind on
    // every config; 16 waves x 1 row — 64 x 4096^2 2.83 vs 1.63 ms, 16384^2 0.66 vs 0.40)
};
constexpr int kNumKeepKernels = sizeof(kKeepKernels) / sizeof(kKeepKernels[0]);
