// gdp_extrema.inc — Scale-space extrema (keypoint) detection on the current pyramid: k_extrema.
// Part of libgdp's single translation unit: included by gdp.hip inside its anonymous namespace
// (after `#pragma clang fp contract(off)`, which therefore applies here too).  Not a header.

// gdp_detect_extrema (gdp.h): levels 0..S+1 of every octave are taken as DoG levels; a candidate
// (s in [1, S], r in [1, rows-2], c in [1, cols-2]) is a keypoint when it is strictly above (kind
// +1) or strictly below (-1) all 26 neighbours, passes |v| > contrast and, when edge_ratio != 0,
// the Hessian edge test.  Read-bound: every level row is loaded once per wave strip.
//
// Work unit = one 64-lane wave: (image, level chunk, octave, tile of kExRows candidate rows, strip
// of kExStrip 4-pixel groups).  Lane l holds group strip * kExStrip - 1 + l: lanes 1..62 own
// candidates, lanes 0 and 63 only carry the halo columns to their neighbours (wave shifts), so
// strips overlap by one group per side and tiles by two rows.  A wave walks down its rows with a
// three-row window of the per-level horizontal 3-max / 3-min; a candidate's own row and level use
// the centre-excluded left/right max.  The max / min are the NaN-propagating ones, so a NaN among
// the 26 neighbours makes both bounds NaN and every comparison false, as a NaN centre does.
// NS = candidate levels a wave keeps in registers (levels base..base+NS+1): S <= 3 in one chunk,
// larger S in chunks of 3 (the last chunk overlaps the one before it and emits only the levels
// that one did not).
constexpr int kExWaves = 4;   // waves (work units) per block
constexpr int kExStrip = 62;  // groups a wave owns candidates of (64 lanes less one halo lane per side)
constexpr int kExRows = 16;   // candidate rows per tile
constexpr int kExStage = 128; // records a wave stages in LDS between two counter atomics (>= 64)

struct ExH {
    f4 a, i;  // horizontal 3-max / 3-min of one level row
};
struct ExC {
    f4 v, la, li;  // a candidate row: the values, max / min of each one's left and right neighbours
};

// lane l gets lane l-1's (up) / lane l+1's (down) value: DPP wave shifts by one lane (gfx9); the
// lane with no source gets 0, which only the halo lanes 0 / 63 ever see
__device__ __forceinline__ float ex_lane_up(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x138 /* wave_shr:1 */, 0xf, 0xf, true));
}
__device__ __forceinline__ float ex_lane_down(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x130 /* wave_shl:1 */, 0xf, 0xf, true));
}

// NaN-propagating max / min (IEEE 754-2019 maximum / minimum; gfx950's v_maximum3_f32 /
// v_minimum3_f32): a NaN anywhere among a candidate's neighbours makes both bounds NaN, which no
// value compares above or below — the rule of gdp.h with no NaN test of its own.
__device__ __forceinline__ f4 ex_max(f4 p, f4 q) { return __builtin_elementwise_maximum(p, q); }
__device__ __forceinline__ f4 ex_min(f4 p, f4 q) { return __builtin_elementwise_minimum(p, q); }
__device__ __forceinline__ f4 ex_max(f4 p, f4 q, f4 r) { return ex_max(ex_max(p, q), r); }
__device__ __forceinline__ f4 ex_min(f4 p, f4 q, f4 r) { return ex_min(ex_min(p, q), r); }

// One level row of a lane's group: the horizontal 3-max / 3-min and, for a candidate level, the
// values with their left/right max / min.
__device__ __forceinline__ void ex_row(f4 x, ExH& h, ExC* c) {
    const f4 l = {ex_lane_up(x.w), x.x, x.y, x.z};    // each pixel's left neighbour
    const f4 r = {x.y, x.z, x.w, ex_lane_down(x.x)};  // and its right one
    if (c) {
        c->v = x;
        c->la = ex_max(l, r);
        c->li = ex_min(l, r);
        h.a = ex_max(c->la, x);
        h.i = ex_min(c->li, x);
    } else {
        h.a = ex_max(l, x, r);
        h.i = ex_min(l, x, r);
    }
}

// The edge-response test of gdp.h on the 3 x 3 patch around q (one level, row pitch `cols`): every
// operation a separately rounded float32 operation, in the documented order.
__device__ __forceinline__ bool ex_edge_ok(const float* __restrict__ q, long long cols, float v, float er) {
    const float dxx = (q[1] + q[-1]) - 2.0f * v;
    const float dyy = (q[cols] + q[-cols]) - 2.0f * v;
    const float dxy = ((q[cols + 1] - q[cols - 1]) - (q[1 - cols] - q[-cols - 1])) * 0.25f;
    const float tr = dxx + dyy;
    const float det = dxx * dyy - dxy * dxy;
    return det > 0.0f && (tr * tr) * er < ((er + 1.0f) * (er + 1.0f)) * det;
}

// One work unit: tile row `tr`, strip `sc` of octave o (geometry og) of image b, levels base ..
// base + NS + 1.  VEC: the octave's width is a multiple of 4, one 16-byte load per group and row;
// otherwise four scalar loads (rows are then not 16-byte aligned).  Loads are branch-free: a group
// or column outside the row is clamped into it — such a pixel is a neighbour of columns 0 and
// cols-1 only, which are no candidates, so its value never matters.
template <int NS, bool VEC>
__device__ __forceinline__ void ex_tile(const OctGeom& og, const float* __restrict__ lev0, uint4* __restrict__ recs,
                                        unsigned* __restrict__ counter, unsigned long long capacity, float thr, float er,
                                        int o, int base, int s_emit, int tr, int sc, int lane, uint4* staged) {
    constexpr int NL = NS + 2;
    const int grp = sc * kExStrip - 1 + lane;
    const int C = 4 * grp;
    const int Cc = 4 * min(max(grp, 0), og.gpr - 1);
    const int cx[4] = {min(max(C, 0), og.cols - 1), min(max(C + 1, 0), og.cols - 1), min(max(C + 2, 0), og.cols - 1),
                       min(max(C + 3, 0), og.cols - 1)};
    auto ld = [&](int l, int r) -> f4 {
        const float* q = lev0 + (long long)l * og.lev_stride + (long long)r * og.cols;
        if constexpr (VEC) return ld_f4(q + Cc);
        return f4{q[cx[0]], q[cx[1]], q[cx[2]], q[cx[3]]};
    };
    // columns this lane may report (bit k: column C + k): inside [1, cols-2], and not a halo lane's
    const bool own = lane >= 1 && lane <= kExStrip;
    unsigned colbits = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) colbits |= (own && C + k >= 1 && C + k <= og.cols - 2) ? 1u << k : 0u;

    // Hits are staged in the wave's own LDS slice and flushed with ONE atomic per kExStage records
    // (and once at the end): the device-wide counter takes a same-address atomic per wave, not per
    // hit.  Only this wave touches the slice and a wave's LDS operations complete in order, so no
    // barrier is needed; n_staged is wave-uniform.
    unsigned n_staged = 0;
    auto flush = [&]() {
        if (n_staged == 0) return;
        unsigned first = 0;
        if (lane == 0) first = atomicAdd(counter, n_staged);
        first = (unsigned)__builtin_amdgcn_readfirstlane((int)first);
        __builtin_amdgcn_wave_barrier();
        for (unsigned i = (unsigned)lane; i < n_staged; i += 64u) {
            const unsigned long long slot = (unsigned long long)first + i;
            if (slot < capacity) recs[slot] = staged[i];
        }
        __builtin_amdgcn_wave_barrier();
        n_staged = 0;
    };
    auto append = [&](bool hit, int kind, int s, int r, int col, float v) {
        if (er != 0.0f && hit)
            hit = ex_edge_ok(lev0 + (long long)(s - base) * og.lev_stride + (long long)r * og.cols + col, og.cols, v, er);
        const unsigned long long mask = __ballot(hit);
        if (mask == 0) return;  // wave-uniform
        const unsigned n_hit = (unsigned)__popcll(mask);
        if (n_staged + n_hit > (unsigned)kExStage) flush();
        const unsigned rank =
            __builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
        if (hit) {
            const unsigned head = (unsigned)o | ((unsigned)s << 16) | (((unsigned)kind & 0xffu) << 24);
            staged[n_staged + rank] = uint4{head, (unsigned)r, (unsigned)col, __float_as_uint(v)};
        }
        n_staged += n_hit;
    };

    // rows [ra, rb) are this tile's candidates; the window holds rows r-1 (up), r (mid), r+1 (cur)
    const int ra = 1 + tr * kExRows;
    const int rb = min(og.rows - 1, ra + kExRows);
    f4 ahead[NL];  // row r + 1 of every level, loaded one step ahead of its use
    auto step = [&](int r, ExH(&up)[NL], ExH(&mid)[NL], ExC(&cen)[NS], ExC(&nxt)[NS]) {
        ExH cur[NL];
        f4 x[NL];
#pragma unroll
        for (int l = 0; l < NL; ++l) x[l] = ahead[l];
#pragma unroll
        for (int l = 0; l < NL; ++l) ahead[l] = ld(l, min(r + 2, rb));  // rb: the last row the tile reads
        __builtin_amdgcn_sched_barrier(0);  // the loads go out before this row's arithmetic, not after it
#pragma unroll
        for (int l = 0; l < NL; ++l) ex_row(x[l], cur[l], (l >= 1 && l <= NS) ? &nxt[l - 1] : nullptr);
        f4 m3a[NL], m3i[NL];  // 3 x 3 max / min of each level around row r
#pragma unroll
        for (int l = 0; l < NL; ++l) {
            m3a[l] = ex_max(up[l].a, mid[l].a, cur[l].a);
            m3i[l] = ex_min(up[l].i, mid[l].i, cur[l].i);
        }
        // hit[4 j + k]: candidate (level base + 1 + j, column C + k) is a keypoint so far (wave masks)
        bool hit[4 * NS], gt[4 * NS], any = false;
        float vals[4 * NS];
#pragma unroll
        for (int j = 0; j < NS; ++j) {
            const int l = j + 1;
            const f4 na = ex_max(m3a[l - 1], m3a[l + 1], ex_max(up[l].a, cur[l].a, cen[j].la));
            const f4 ni = ex_min(m3i[l - 1], m3i[l + 1], ex_min(up[l].i, cur[l].i, cen[j].li));
            const float v4[4] = {cen[j].v.x, cen[j].v.y, cen[j].v.z, cen[j].v.w};
            const float a4[4] = {na.x, na.y, na.z, na.w};
            const float i4[4] = {ni.x, ni.y, ni.z, ni.w};
            const unsigned ok = base + l > s_emit ? colbits : 0u;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                gt[4 * j + k] = v4[k] > a4[k];
                hit[4 * j + k] = (gt[4 * j + k] || v4[k] < i4[k]) && fabsf(v4[k]) > thr && ((ok >> k) & 1u);
                any = any || hit[4 * j + k];
                vals[4 * j + k] = v4[k];
            }
        }
        // the rare part: every lane reports its hits one at a time, lowest bit first
        if (__ballot(any) != 0) {  // wave-uniform
            unsigned hits = 0, maxima = 0;
#pragma unroll
            for (int q = 0; q < 4 * NS; ++q) {
                hits |= hit[q] ? 1u << q : 0u;
                maxima |= gt[q] ? 1u << q : 0u;
            }
            do {
                const bool mine = hits != 0;
                const int bit = mine ? __ffs((int)hits) - 1 : 0;
                float v = vals[0];
#pragma unroll
                for (int q = 1; q < 4 * NS; ++q) v = bit == q ? vals[q] : v;
                append(mine, (maxima >> bit) & 1u ? 1 : -1, base + 1 + (bit >> 2), r, C + (bit & 3), v);
                hits &= hits - 1u;
            } while (__ballot(hits != 0) != 0);
        }
#pragma unroll
        for (int l = 0; l < NL; ++l) up[l] = cur[l];
    };

    ExH A[NL], B[NL];
    ExC P[NS], Q[NS];
#pragma unroll
    for (int l = 0; l < NL; ++l) ex_row(ld(l, ra - 1), A[l], nullptr);
#pragma unroll
    for (int l = 0; l < NL; ++l) ex_row(ld(l, ra), B[l], (l >= 1 && l <= NS) ? &P[l - 1] : nullptr);
#pragma unroll
    for (int l = 0; l < NL; ++l) ahead[l] = ld(l, ra + 1);
    for (int r = ra; r < rb; r += 2) {
        step(r, A, B, P, Q);
        if (r + 1 < rb) step(r + 1, B, A, Q, P);
    }
    flush();
}

template <int NS>
__global__ void __launch_bounds__(64 * kExWaves) k_extrema(const Geom* __restrict__ g, const float* __restrict__ pyr,
                                                           uint4* __restrict__ recs, unsigned* __restrict__ count,
                                                           unsigned long long capacity, float thr, float er,
                                                           unsigned nchunks) {
    __shared__ uint4 ex_stage[kExWaves][kExStage];
    const int lane = (int)(threadIdx.x & 63u);
    const unsigned wave = (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const unsigned per = g->ex_blk[g->O];  // units per image and level chunk
    const unsigned per_img = per * nchunks;
    const unsigned u = blockIdx.x * kExWaves + wave;
    if (u >= per_img * (unsigned)g->batch) return;  // wave-uniform
    const unsigned b = u / per_img;
    const unsigned rem = u - b * per_img;
    const unsigned ch = rem / per;
    const unsigned w = rem - ch * per;
    int o = 0;
    while (o + 1 < g->O && w >= g->ex_blk[o + 1]) ++o;
    const OctGeom og = g->oct[o];
    const unsigned strips = (unsigned)g->ex_strips[o];
    const unsigned t = w - g->ex_blk[o];
    const int tr = (int)(t / strips);
    const int sc = (int)(t - (unsigned)tr * strips);
    const int base = min((int)(ch * NS), g->S - NS);  // levels base .. base + NS + 1
    const int s_emit = (int)(ch * NS);                // candidate levels s > s_emit are this chunk's
    const float* lev0 = pyr + (long long)b * g->pyr_stride + og.lev_off + (long long)base * og.lev_stride;
    uint4* const out = recs + (unsigned long long)b * capacity;
    if ((og.cols & 3) == 0)
        ex_tile<NS, true>(og, lev0, out, count + b, capacity, thr, er, o, base, s_emit, tr, sc, lane, ex_stage[wave]);
    else
        ex_tile<NS, false>(og, lev0, out, count + b, capacity, thr, er, o, base, s_emit, tr, sc, lane, ex_stage[wave]);
}
