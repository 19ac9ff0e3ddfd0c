// gdp_build.inc — k_build: the fused GaussPyInit + GenerateDoG kernel and its code variants.
// Part of libgdp's single translation unit: included by gdp.hip inside its anonymous namespace
// (after `#pragma clang fp contract(off)`, which therefore applies here too).  Not a header.

// One group = 4 consecutive output pixels (Rl, C..C+3) of octave o, all S+3 scales.
// G_s = (x * fc_s) * fr_s ; out_s = G_s - G_{s+1} ; out_{L-1} = G_{L-1}.
// SUB: GaussPyramid_a512omp::GenerateDoG_nomp_dynamic's output instead
// (GaussDePyramid-AVX512xOpenMP.h:240-364): only scales 0..S-1 are windowed (:242-318, row pass
// then column pass, so the same (x * fc_s) * fr_s), DoG only for s < S-1 (:337-357), and levels
// S..S+2 keep GaussPyInit's value x.
// `keep` != 0 (never for SUB, whose levels S..S+2 hold x): the context's pyramid already holds the
// input-independent +0 of every DoG level outside the windows' support, so those stores are skipped.
template <int LT, bool NT, bool SUB = false>
__device__ __forceinline__ void build_group(const Geom* __restrict__ g, const void* __restrict__ in,
                                            float* __restrict__ out, const float* __restrict__ taps, int keep,
                                            int b, int o, const OctGeom& og, int Rl, int C) {
    const int L = LT > 0 ? LT : g->L;
    const int n = min(4, og.cols - C);
    const int Rg = og.row0 + Rl;
    const f4 x = load_px(g, in, b, o, Rg, C, n);
    const float* ct = taps + og.ctap + C;
    const float* rt = taps + og.rtap + Rg * og.rtap_row;
    // column / row window of scale s
    auto fc = [&](int s) -> f4 { return ld_f4(ct + s * og.ctap_stride); };
    auto fr = [&](int s) -> float { return rt[s * og.rtap_stride]; };
    float* dst = out + (long long)b * g->pyr_stride + og.lev_off + (long long)Rl * og.cols + C;
    const bool full = (n == 4) && ((og.cols & 3) == 0);
    if constexpr (SUB) {
        const int Sw = L - 3; // windowed scales (S; compile-time when LT is)
        const int pace = g->store_pace;
        f4 gp = Sw > 0 ? (x * fc(0)) * fr(0) : x;
#pragma unroll
        for (int s = 0; s + 1 < L; ++s) {
            const bool wn = s + 1 < Sw; // level s+1 windowed, and level s = G_s - G_{s+1}
            const f4 gn = wn ? (x * fc(s + 1)) * fr(s + 1) : x;
            const f4 d = wn ? gp - gn : gp;
            if (full)
                st_f4<NT>(dst + s * og.lev_stride, d);
            else
                st_part(dst + s * og.lev_stride, d, n, false);
            pace_stores(pace);
            gp = gn;
        }
        if (full)
            st_f4<NT>(dst + (L - 1) * og.lev_stride, gp);
        else
            st_part(dst + (L - 1) * og.lev_stride, gp, n, false);
        return;
    }
    if (keep && outside_support(og, Rg, C, n)) {
        // Clean pyramid (gdp_ctx::zeros_clean; `keep` is a wave-uniform kernel argument): outside the
        // TRUE support (OctGeom::sp_*, whatever GDP_TUNE_ZERO_WINDOW says) the S+2 DoG levels are +0
        // for any input, and an earlier build of this context already stored exactly that — nothing
        // has written the pyramid since.  Only level L-1 = copysign(0, x) depends on the image: one
        // load, one store, no window loads and no pace wait.
        const f4 last = __builtin_bit_cast(f4, __builtin_bit_cast(i4, x) & (int)0x80000000u);
        if (full)
            st_f4<NT>(dst + (L - 1) * og.lev_stride, last);
        else
            st_part(dst + (L - 1) * og.lev_stride, last, n, false);
        return;
    }
    if (zero_support(og, Rg, C, n)) {
        // Outside the support of every window (GDP_TUNE_ZERO_WINDOW; OctGeom::nz_*): the row's or
        // all four columns' taps are +0 for every scale, so each G_s = (x * fc) * fr is a zero
        // carrying x's sign (taps are >= +0).  The DoG levels G_s - G_{s+1} are then +0 whatever
        // x is — stored without waiting for the load — and level L-1 = G_{L-1} is copysign(0, x).
        // No window loads and no multiplies.  Measured (profiles/zw*_r03a{i,j}.log): 2-4 % faster
        // on 16384^2, whose window lines are cold, but 7-15 % slower on 4096^2 and on batches: the
        // full path's level-(s+1) window loads between its stores pace them (about one store in
        // flight per wave, the write path's best rate), and forming the zeros as x - x so the
        // stores wait for the input does not restore that — hence a tuning knob in the autotune.
        const f4 z = {0.f, 0.f, 0.f, 0.f};
        const int pace = g->store_pace;
        for (int s = 0; s + 1 < L; ++s) {
            if (full)
                st_f4<NT>(dst + s * og.lev_stride, z);
            else
                st_part(dst + s * og.lev_stride, z, n, false);
            pace_stores(pace);
        }
        const f4 last = __builtin_bit_cast(f4, __builtin_bit_cast(i4, x) & (int)0x80000000u);
        if (full)
            st_f4<NT>(dst + (L - 1) * og.lev_stride, last);
        else
            st_part(dst + (L - 1) * og.lev_stride, last, n, false);
        return;
    }
    const int pace = g->store_pace;
    f4 gp = (x * fc(0)) * fr(0);
#pragma unroll
    for (int s = 0; s + 1 < L; ++s) {
        const f4 gn = (x * fc(s + 1)) * fr(s + 1);
        const f4 d = gp - gn;
        if (full)
            st_f4<NT>(dst + s * og.lev_stride, d);
        else
            st_part(dst + s * og.lev_stride, d, n, false);
        pace_stores(pace);
        gp = gn;
    }
    if (full)
        st_f4<NT>(dst + (L - 1) * og.lev_stride, gp);
    else
        st_part(dst + (L - 1) * og.lev_stride, gp, n, false);
}

// Tail unit `tu` (0-based): 256 consecutive groups of the tiny octaves >= F, flattened over the
// batch, one group per thread.  (Measured and dropped, round 3: a tile order with each image's
// tail units right after its own tiles, so they read input lines still on chip instead of at the
// end of the grid — bit-exact, ±1 %: config 3 v11 0.6945 vs 0.6904 ms, v16 0.713 vs 0.720, config
// 2 v16 0.0861 vs 0.0857, config 4 v16 5.38 vs 5.40; profiles/ab_tail_c*_r03z.log.)
template <int LT, bool NT, int BLK, bool SUB>
__device__ __forceinline__ void build_tail_unit(const Geom* __restrict__ g, const void* __restrict__ in,
                                                float* __restrict__ out, const float* __restrict__ taps, int keep,
                                                unsigned tu) {
    const int F = g->F;
    for (int q = threadIdx.x; q < kTailGroups; q += BLK) {
        const unsigned t = tu * kTailGroups + q;
        const unsigned per = g->tail_groups_per_img;
        if (t >= per * (unsigned)g->batch) break;
        const unsigned b = t / per;
        const long long rem = (long long)(t - b * per) + g->oct[F].grp_begin;
        int o = F;
        while (o + 1 < g->O && rem >= g->oct[o + 1].grp_begin) ++o;
        const OctGeom og = g->oct[o];
        const int k = (int)(rem - og.grp_begin);
        const int Rl = k / og.gpr;
        const int C = 4 * (k - Rl * og.gpr);
        build_group<LT, NT, SUB>(g, in, out, taps, keep, (int)b, o, og, Rl, C);
    }
}

// Fused build.  Work units: [0, tiles_total) are 16 x 256 input tiles (octaves 0..F-1 of the
// tile: octave o covers (16>>o) rows x (256>>o) columns, reading lines the o = 0 pass of the
// same block just brought on chip); [tiles_total, +tail_units) are 256-group slices of the tiny
// octaves >= F.  Default launch: one unit per block (the dispatcher back-fills CUs as blocks
// retire, which measured faster than a persistent grid); the grid-stride loop serves capped grids.
// BLK = threads per block; PATH 0 = generic loop (thread q takes groups q, q+BLK, .. of each
// octave in turn), 3 = octave 0 then octaves 1.. flattened into one second round, 4 / 5 =
// contiguous spans (below).  (PATH 1, register-resident octave 0 on 256 threads, and PATH 2, one
// group per thread across all fused octaves, were measured slower everywhere and removed in
// round 5 with the variants that used them — DESIGN_HISTORY §4.)
template <int LT, bool NT, int BLK, int TC, int PATH, int TR, bool SUB>
__device__ __forceinline__ void build_body(const Geom* __restrict__ g, const void* __restrict__ in,
                                           float* __restrict__ out, const float* __restrict__ taps, int keep) {
    const unsigned tiles_total = g->tiles_total;
    const unsigned units = tiles_total + g->tail_units;
    const int F = g->F;
    for (unsigned u = blockIdx.x; u < units; u += gridDim.x) {
        if (u < tiles_total) {
            // tile order: 0 = linear; 1 = XCD-chunked (blocks b and b+8 share an XCD under the
            // observed round-robin dispatch, so XCD x walks the contiguous tile range x/8 of the
            // grid) — a speed knob only, any order gives the same bits
            unsigned t = u;
            if (g->tile_order == 1 && (tiles_total & 7u) == 0) {
                t = (u & 7u) * (tiles_total >> 3) + (u >> 3);
            } else if (g->tile_order == 2 && ((tiles_total / (unsigned)g->tiles_c) & 7u) == 0) {
                // XCD row-interleave: XCD x sweeps whole tile rows x, x+8, ... left to right
                const unsigned k = u >> 3, tcs = (unsigned)g->tiles_c;
                const unsigned q = k / tcs;
                t = (q * 8u + (u & 7u)) * tcs + (k - q * tcs);
            }
            const unsigned b = t / g->tiles_per_img;
            const unsigned rem = t - b * g->tiles_per_img;
            if constexpr (PATH == 4 || PATH == 5) {
                // Contiguous spans (retile, tile_rows == 0): unit `rem` of image b owns groups
                // [rem * span_o, (rem + 1) * span_o) of EVERY octave o in row-major order, so each
                // wave store continues where the previous lane's ended, across row boundaries, and
                // the unit writes one contiguous run of every level.  Octave 0 takes TC / BLK
                // rounds of one group per thread; octaves 1.. are flattened into one more round
                // (PATH 3's shape).  The octave-o chunk decimates the input rows octave 0's chunk
                // just read (proportional cuts), so those loads hit lines already on chip.
                {
                    const OctGeom og = g->oct[0];
                    const unsigned total = (unsigned)og.rows * (unsigned)og.gpr;
                    const unsigned lo = rem * (unsigned)og.span;
#pragma unroll
                    for (int q0 = 0; q0 < TC; q0 += BLK) {
                        const unsigned q = (unsigned)q0 + threadIdx.x;
                        if (q >= (unsigned)og.span || lo + q >= total) break;
                        const int Rl = (int)fast_div(lo + q, og.gpr_magic, og.gpr_shift);
                        const int C = 4 * (int)(lo + q - (unsigned)Rl * (unsigned)og.gpr);
                        build_group<LT, NT, SUB>(g, in, out, taps, keep, (int)b, 0, og, Rl, C);
                    }
                }
                if constexpr (PATH == 4) {
                    for (int q = (int)threadIdx.x; q < g->span_rest; q += BLK) {
                        int o = 1, qq = q;
                        while (o < g->O && qq >= g->oct[o].span) {
                            qq -= g->oct[o].span;
                            ++o;
                        }
                        if (o >= g->O) break;
                        const OctGeom og = g->oct[o];
                        const unsigned grp = rem * (unsigned)og.span + (unsigned)qq;
                        if (grp >= (unsigned)og.rows * (unsigned)og.gpr) continue;
                        const int Rl = (int)fast_div(grp, og.gpr_magic, og.gpr_shift);
                        const int C = 4 * (int)(grp - (unsigned)Rl * (unsigned)og.gpr);
                        build_group<LT, NT, SUB>(g, in, out, taps, keep, (int)b, o, og, Rl, C);
                    }
                } else {
                    // PATH 5, source-aligned: octave o's groups whose first input pixel (r << o,
                    // C << o) lies in THIS unit's octave-0 chunk [a, e) — a contiguous run of the
                    // octave-o level too (the group -> source map is monotone), every input line it
                    // reads one this unit just loaded (no neighbour's lines, whatever the order).
                    // first_of(r, c): octave-o groups with source before input pixel (r, c).
                    const OctGeom o0 = g->oct[0];
                    const unsigned total0 = (unsigned)o0.rows * (unsigned)o0.gpr;
                    const unsigned a = min(rem * (unsigned)o0.span, total0);
                    const unsigned e = min(a + (unsigned)o0.span, total0);
                    const unsigned ra = fast_div(a, o0.gpr_magic, o0.gpr_shift), ca = 4u * (a - ra * (unsigned)o0.gpr);
                    const unsigned re = fast_div(e, o0.gpr_magic, o0.gpr_shift), ce = 4u * (e - re * (unsigned)o0.gpr);
                    unsigned base = 0;  // items of octaves 1 .. o-1 before octave o's, flattened over the threads
                    for (int o = 1; o < g->O; ++o) {
                        const OctGeom og = g->oct[o];
                        auto first_of = [&](unsigned r, unsigned c) -> unsigned {
                            const unsigned step = 1u << o;
                            unsigned n = min((unsigned)og.rows, (r + step - 1) >> o) * (unsigned)og.gpr;
                            if ((r & (step - 1)) == 0 && (r >> o) < (unsigned)og.rows)
                                n += min((unsigned)og.gpr, (c + (4u << o) - 1) / (4u << o));
                            return n;
                        };
                        const unsigned lo = first_of(ra, ca), cnt = first_of(re, ce) - lo;
                        // this thread's items idx == threadIdx.x (mod BLK) in [base, base + cnt)
                        unsigned idx = base + (threadIdx.x + BLK - base % BLK) % BLK;
                        for (; idx < base + cnt; idx += BLK) {
                            const unsigned grp = lo + (idx - base);
                            const int Rl = (int)fast_div(grp, og.gpr_magic, og.gpr_shift);
                            const int C = 4 * (int)(grp - (unsigned)Rl * (unsigned)og.gpr);
                            build_group<LT, NT, SUB>(g, in, out, taps, keep, (int)b, o, og, Rl, C);
                        }
                        base += cnt;
                    }
                }
                continue;
            }
            const unsigned tr = rem / (unsigned)g->tiles_c;
            const unsigned tc = rem - tr * (unsigned)g->tiles_c;
            const int in_r0 = (int)tr * TR; // band-local input row of the tile
            const int in_c0 = (int)tc * TC;
            constexpr int kFusedT = TR == 16 ? 5 : TR == 8 ? 4 : TR == 4 ? 3 : TR == 2 ? 2 : 1; // log2(TR)+1
            if constexpr (PATH == 3) {
                // Two rounds per block: octave 0 one group per thread, then octaves 1..F-1
                // FLATTENED over the threads (16 x 256: 340 groups on waves 0-5), instead of one
                // octave after another on the first waves — no wave lives more than two rounds,
                // so a block's wave slots free together (PATH 0: wave 0 serially does octaves 0-4
                // while the other waves' slots sit empty until the block retires).
                constexpr int kRest = [] {
                    int n = 0;
                    for (int k = 1; k < kFusedT; ++k) n += (TR >> k) * ((TC / 4) >> k);
                    return n;
                }();
                // (measured and dropped, round 3: every window — and the input — of a thread's
                // two groups loaded before its first store, so no window load waits behind stores
                // in the in-order vmcnt: slower everywhere, e.g. cold 4096^2 v15 0.096-0.124 vs
                // 0.084 ms, 64 x 4096^2 5.6-8.2 vs 5.3 ms, 65536 x 4096 1.38-1.94 vs 1.38-1.40 ms;
                // profiles/ab_preload_r03a.log)
                {
                    const OctGeom og = g->oct[0];
                    constexpr int gpr_t = TC / 4;
#pragma unroll
                    for (int q0 = 0; q0 < TR * gpr_t; q0 += BLK) {
                        const int q = q0 + (int)threadIdx.x;
                        if (q >= TR * gpr_t) break;
                        const int r = q / gpr_t, cg = q - r * gpr_t;
                        const int Rl = in_r0 + r, C = in_c0 + 4 * cg;
                        if (Rl < og.rows && C < og.cols) build_group<LT, NT, SUB>(g, in, out, taps, keep, (int)b, 0, og, Rl, C);
                    }
                }
                for (int q = (int)threadIdx.x; q < kRest; q += BLK) {
                    int o = 1, qq = q;
#pragma unroll
                    for (int k = 1; k < kFusedT; ++k) {
                        const int gk = (TR >> k) * ((TC / 4) >> k);
                        if (o == k && qq >= gk) {
                            qq -= gk;
                            o = k + 1;
                        }
                    }
                    if (o >= F) continue;
                    const OctGeom og = g->oct[o];
                    const int gpr_t = (TC / 4) >> o;
                    const int r = qq / gpr_t, cg = qq - r * gpr_t;
                    const int Rl = (in_r0 >> o) + r, C = (in_c0 >> o) + 4 * cg;
                    if (Rl < og.rows && C < og.cols) build_group<LT, NT, SUB>(g, in, out, taps, keep, (int)b, o, og, Rl, C);
                }
                continue;
            }
#pragma unroll
            for (int o = 0; o < kFusedT; ++o) {
                if (o >= F) break;
                const OctGeom og = g->oct[o];
                const int gpr_t = (TC / 4) >> o; // groups per tile row (TC = 256: 64, 32, 16, 8, 4)
                const int groups = (TR >> o) * gpr_t;
#pragma unroll
                for (int q0 = 0; q0 < groups; q0 += BLK) {
                    const int q = q0 + (int)threadIdx.x;
                    if (q >= groups) break;
                    const int r = q / gpr_t;
                    const int cg = q - r * gpr_t;
                    // band-local output row: in_row0 is a multiple of 16, so local input row
                    // in_r0 + (r << o) maps to local output row (in_r0 >> o) + r.
                    const int Rl = (in_r0 >> o) + r;
                    const int C = (in_c0 >> o) + 4 * cg;
                    if (Rl < og.rows && C < og.cols) build_group<LT, NT, SUB>(g, in, out, taps, keep, (int)b, o, og, Rl, C);
                }
            }
        } else {
            build_tail_unit<LT, NT, BLK, SUB>(g, in, out, taps, keep, u - tiles_total);
        }
    }
}

#ifdef GDP_TRACE_BLOCKS
// Diagnostic build only (tools/trace/): per wave, the 100 MHz real-time clock at entry and after
// the wave's last store was issued, and the XCC / CU it ran on — to see a launch's ramp and tail.
// Per WAVE, no barrier (a __syncthreads here waits for every store of the block to be
// acknowledged and doubles the launch time — waves normally retire with stores in flight).
__device__ unsigned long long* g_block_trace = nullptr;
__device__ __forceinline__ void trace_wave(unsigned long long t_in, int waves_per_block) {
    if ((threadIdx.x & 63) == 0 && g_block_trace) {
        unsigned xcc, hw;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
        unsigned long long* p =
            g_block_trace + 3ull * ((unsigned long long)blockIdx.x * waves_per_block + (threadIdx.x >> 6));
        p[0] = t_in;
        p[1] = __builtin_amdgcn_s_memrealtime();
        p[2] = ((unsigned long long)xcc << 32) | hw;
    }
}
#endif

template <int LT, bool NT, int BLK, int TC, int PATH, int TR, bool SUB = false>
__global__ void __launch_bounds__(BLK) k_build(const Geom* __restrict__ g, const void* __restrict__ in,
                                               float* __restrict__ out, const float* __restrict__ taps, int keep) {
#ifdef GDP_TRACE_BLOCKS
    const unsigned long long t_in = __builtin_amdgcn_s_memrealtime();
#endif
    build_body<LT, NT, BLK, TC, PATH, TR, SUB>(g, in, out, taps, keep);
#ifdef GDP_TRACE_BLOCKS
    trace_wave(t_in, BLK / 64);
#endif
}

// Build-kernel code variants (GDP_TUNE_VARIANT); all bit-identical, A/B'd by tools/tune.py.
// ksub: the same tile shape computing GenerateDoG_nomp_dynamic's subset (gdp_build_subset).
// `id` is the variant's number since round 1 (bench logs and PMC records name variants by it);
// round 5 kept only the ids an autotune picked on some config in round 4 (bench_*_r04*.log: 0, 8,
// 15, 16, 17, 18, 20, 23, 27) plus 11, the 1920-wide default on a hipMalloc'd pyramid
// (default_variant).  The other 20 were never selected and are gone (DESIGN_HISTORY §4 has their
// numbers): GDP_TUNE_VARIANT refuses their ids.
struct BuildVariant {
    int id, block, tile_cols, tile_rows;
    void (*k[2][2])(const Geom*, const void*, float*, const float*, int); // [LT==5][NT]
    void (*ksub[2][2])(const Geom*, const void*, float*, const float*, int); // [LT==5][NT]
};
#define GDP_VARIANT(ID, BLK, TC, REG, TR)                                                         \
    BuildVariant {                                                                                \
        ID, BLK, TC, TR, {{k_build<0, false, BLK, TC, REG, TR>, k_build<0, true, BLK, TC, REG, TR>}, \
                          {k_build<5, false, BLK, TC, REG, TR>, k_build<5, true, BLK, TC, REG, TR>}}, \
            {{k_build<0, false, BLK, TC, REG, TR, true>, k_build<0, true, BLK, TC, REG, TR, true>},  \
             {k_build<5, false, BLK, TC, REG, TR, true>, k_build<5, true, BLK, TC, REG, TR, true>}}   \
    }
const BuildVariant kVariants[] = {
    GDP_VARIANT(0, 1024, 256, 0, 16),  // 16 waves, one octave-0 group per thread; octaves 1-4 serially on the first waves
    GDP_VARIANT(8, 512, 256, 0, 8),    // 8 waves, 8 x 256 tile (octaves 0-3 fused)
    GDP_VARIANT(11, 768, 384, 0, 8),   // 12 waves, 8 x 384 tile (W = 1920: 5 tiles, H = 1080: 135)
    GDP_VARIANT(15, 1024, 256, 3, 16), // (default) v0's tile, octaves 1-4 flattened into one second round
    GDP_VARIANT(16, 512, 256, 3, 8),   // v8's tile, octaves 1-3 flattened
    GDP_VARIANT(17, 768, 384, 3, 8),   // v11's tile, octaves 1-3 flattened
    GDP_VARIANT(18, 512, 128, 3, 16),  // 8 waves, 16 x 128 tile, octaves 1-4 flattened
    // contiguous spans (PATH 4, tile_rows 0): block threads, octave-0 groups per unit (x 16 B per level)
    GDP_VARIANT(20, 512, 512, 4, 0),   // 8 KiB of every octave-0 level per unit, 8 waves
    GDP_VARIANT(23, 768, 768, 4, 0),   // 12 KiB per unit, 12 waves
    // source-aligned spans (PATH 5): octave o's chunk = the groups decimating this unit's own input
    GDP_VARIANT(27, 512, 512, 5, 0),   // v20's unit
    // (measured and dropped, round 3: 4-wave blocks, flattened, on 16 x 64 / 8 x 128 tiles — the
    // shape that helps the in-place passes — config 2 0.107 / 0.091 vs 0.083-0.084 ms, config 4 6.91 /
    // 5.64 vs 4.85-5.17, config 5 1.45 / 1.36 vs 1.29, config 3 0.83 / 0.74 vs 0.69;
    // profiles/ab_small_c*_r03p.log)
    // (measured and dropped, round 3: whole-row tiles, so a block's stores are one contiguous span
    // per level instead of rows 7,680 B apart — 960 x 2x1920, 960 x 4x1920, 480 x 2x960,
    // 960 x 4x960: config 3 0.783 / 0.859 / 0.774 / 0.798 vs 0.694 ms for v11, config 2 0.127 /
    // 0.094 (4x1920 / 4x960) vs 0.085, config 4 7.18 / 6.03 vs 5.20; profiles/rowtile_c*_r03ah.log)
    // (measured and dropped, round 3: the flattened form of every other tile that divides 1920 —
    // 768 x 16x192, 640 x 8x320 (3 blocks / 30 waves per CU), 960 x 8x480 — config 3 0.829 / 0.731 /
    // 0.875 vs 0.685 ms for v11, config 2 0.091 / 0.087 / 0.091 vs 0.084-0.085, config 4 6.08 /
    // 5.57 / 6.06 vs 5.08-5.26; profiles/ab_c{2,3,4}_r03i.log)
    // (measured and dropped: the 16 x 256 tile on 8 or 4 waves, 3 or 6 rounds for the first
    // waves — 0.103 / 0.124 ms; 16 x 128 on 4 waves, 3 rounds — 0.109: every round beyond the
    // second costs a store latency, since gfx9's one in-order vmcnt makes the next round's loads
    // wait for the previous round's stores)
    // (measured and dropped: PATH 2 on a 16 x 192 tile — one group per thread over all five
    // octaves, 1,023 groups, one round of 16 waves — 0.107 vs 0.083 ms for v15 on a cold 4096^2)
    // (measured and dropped, round 2: v15's tile with octave 0 register-resident on 8 or 4 waves,
    // every input load of a thread before its first store, octaves 1-4 flattened — 2 / 4 rows per
    // wave: cold 4096^2 0.0952 / 0.1068 vs 0.0856 ms for v15, 64 x 4096^2 5.61 / 6.14 vs 5.25,
    // 16384^2 1.331 / 1.520 vs 1.332; profiles/ab_path4_c*_r02ah.log — fewer waves keep fewer
    // stores in flight, and issuing the loads first does not buy that back)
    // (measured and dropped: PATH 2 on 16 x 128 / 16 x 64 / 8 x 128 / 4 x 256 / 8 x 64 tiles —
    // all slower; PATH 2 itself is 25-50 % slower than v0 on batches and 16384^2)
};

// Default variant for a width and pyramid backing (tools/tune.py, MI355X, cold buffers) — the
// one place the default is decided.  Where the width fills 256-wide tiles: v15 — v0's 1024
// threads on 16 x 256 tiles with octaves 1-4 flattened into one second round (PATH 3), so no wave
// lives more than two rounds and a block's wave slots free together: single 4096^2 image
// 0.0852-0.0853 vs 0.0902-0.0907 ms for v0, 16384^2 1.344 vs 1.354-1.434, 64 x 4096^2 equal to
// v0.  When a 256-wide tile grid would leave lanes idle, the tile width with the fewest idle
// lanes: 8 x 384 tiles (W = 1920: 5 tiles) — flattened (v17) on the default chunked backing
// (64 x 1080x1920 0.637 vs 0.698 ms for v11, profiles/defvar_c3_r04am.log), v11 on one hipMalloc
// (0.68-0.69 vs 0.78 for v17, round 3) — else 16 x 128 tiles (v18).  gdp_autotune measures all.
int default_variant(int W, bool chunked) {
    const long long waste256 = (long long)((W + 255) / 256) * 256 - W;
    const long long waste384 = (long long)((W + 383) / 384) * 384 - W;
    const long long waste128 = (long long)((W + 127) / 128) * 128 - W;
    // compare idle-lane fractions of a tile row (waste / tile width), 256 preferred on ties
    if (waste256 * 384 > waste384 * 256 && waste384 * 128 <= waste128 * 384) return chunked ? 17 : 11;
    if (waste256 * 128 > waste128 * 256) return 18;
    return 15;
}
constexpr int kNumVariants = sizeof(kVariants) / sizeof(kVariants[0]);
// index into kVariants of variant `id`, -1 if no such variant is built
int variant_index(int id) {
    for (int i = 0; i < kNumVariants; ++i)
        if (kVariants[i].id == id) return i;
    return -1;
}
