// gdp_orient.inc — Keypoint orientation assignment on the current pyramid: k_orient.
// Part of libgdp's single translation unit: included by gdp.hip inside its anonymous namespace
// (after `#pragma clang fp contract(off)`, which therefore applies here too).  Not a header.

// gdp_orient_keypoints (gdp.h): for every refined record (o, s, r, c) the Gaussian level
// L = P[S+2] + P[S+1] + ... + P[s] is rebuilt around the sample (the DoG levels telescope), the
// gradients of a (2R+1)^2 window go into a 36-bin histogram weighted by a Gaussian of the distance,
// the histogram is smoothed and every peak within 80 % of the highest becomes one 48-byte record.
// Every operation is the separately rounded float32 operation gdp.h writes down, in its order; the
// square root and the division are IEEE-correct (sqrtf, plain `/`).
//
// One 16-lane DPP row per input record, four records per wave, 256-thread blocks over batch x
// ceil(inputs / 16).  Lane i of a row owns image row r - R - 1 + i (2R + 3 <= 13 lanes live): it
// rebuilds its row of L over columns c - R - 1 .. c + R + 1 in registers (addresses clamped into the
// level: a clamped value is only ever a neighbour of a sample the rule skips), takes the rows above
// and below from its neighbour lanes (row_shr:1 / row_shl:1) and adds its 2R + 1 samples in
// ascending dc into its own 36-float LDS slice — the rule's per-row partial, no atomics.  The row's
// lanes then add the slices in ascending dr (lane j: bins j, j + 16, j + 32), smooth, and find the
// peaks; the records are compacted per wave as k_extrema and k_refine do (ballot + mbcnt rank, one
// atomic per wave).  Everything between lanes goes through the wave's own LDS, whose operations
// complete in order: no block barrier.
constexpr int kOrBlock = 256;
constexpr int kOrGroup = 16;                             // lanes per record: one DPP row
constexpr int kOrPerBlock = kOrBlock / kOrGroup;         // records per block
constexpr int kOrBins = 36;
constexpr int kOrMaxR = 5;                               // radius of scale 1, the largest
constexpr int kOrCols = 2 * kOrMaxR + 3;                 // columns (and rows) of L a record reads at most
constexpr int kOrWeights = 2 * kOrMaxR * kOrMaxR + 1;    // w_s[d2], d2 = 0 .. 2 R^2: floats per scale
constexpr int kOrSlice = kOrBins + 1;                    // a lane's LDS slice, padded: a row's lanes read
                                                         // consecutive bins of one slice conflict-free
constexpr unsigned kOrNoList = 0xffffffffu;              // own_count[b]: image b reads the context's refined list
static_assert(sizeof(gdp_keypoint_oriented) == 48 && sizeof(gdp_keypoint_refined) == 32, "three / two 16-byte words per record");

// ceil(3 * 1.5 * sigma_s), sigma_s = 2 / (s + 1): 5, 3, 3, 2, 2, 2, 2, 1, ...
__host__ __device__ __forceinline__ int or_radius(int s) { return (9 + s) / (s + 1); }

// lane l gets lane l-1's (up) / lane l+1's (down) value within its 16-lane row; a lane with no source
// gets 0, which only lanes that own no sample ever see
__device__ __forceinline__ float or_lane_up(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x111 /* row_shr:1 */, 0xf, 0xf, true));
}
__device__ __forceinline__ float or_lane_down(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x101 /* row_shl:1 */, 0xf, 0xf, true));
}

// The bin of gdp.h: the quadrant, then the number of the eight 10-degree boundaries inside it that
// (ax, ay) has passed; T[k] is the float32 nearest to tan(k * 10 degrees).
__device__ __forceinline__ int or_bin(float gx, float gy) {
    int q;
    float ax, ay;
    if (gx > 0.0f && gy >= 0.0f) {
        q = 0, ax = gx, ay = gy;
    } else if (gx <= 0.0f && gy > 0.0f) {
        q = 1, ax = gy, ay = -gx;
    } else if (gx < 0.0f && gy <= 0.0f) {
        q = 2, ax = -gx, ay = -gy;
    } else {
        q = 3, ax = -gy, ay = gx;
    }
    constexpr unsigned T[8] = {0x3e348f0fu, 0x3eba5a4eu, 0x3f13cd3au, 0x3f56cf3cu,
                               0x3f988b62u, 0x3fddb3d7u, 0x402fd6acu, 0x40b57b24u};
    int j = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) j += (int)(ay >= ax * __uint_as_float(T[k]));
    return 9 * q + j;
}

__global__ void __launch_bounds__(kOrBlock) k_orient(const Geom* __restrict__ g, const float* __restrict__ pyr,
                                                     const uint4* __restrict__ rf, const unsigned* __restrict__ rf_count,
                                                     unsigned long long rf_capacity, const uint4* __restrict__ own,
                                                     const unsigned* __restrict__ own_count,
                                                     const float* __restrict__ weights, uint4* __restrict__ recs_out,
                                                     unsigned* __restrict__ count_out, unsigned long long capacity,
                                                     unsigned blocks_per_img) {
    __shared__ float or_part[kOrBlock / 64][64][kOrSlice];       // per lane: its window row's partial histogram
    __shared__ float or_hist[kOrBlock / 64][4][2][kOrBins + 4];  // per record: the histogram, then the smoothed one
    const unsigned b = blockIdx.x / blocks_per_img;
    const unsigned long long first = (unsigned long long)(blockIdx.x - b * blocks_per_img) * kOrPerBlock;
    // the list: the caller's (gdp_orient_set_input) or the context's refined one; block-uniform
    const unsigned n_own = own_count[b];
    const unsigned long long n = n_own != kOrNoList ? (unsigned long long)n_own : min((unsigned long long)rf_count[b], rf_capacity);
    if (first >= n) return;
    const uint4* const src = n_own != kOrNoList ? own + 2ull * b * capacity : rf + 2ull * b * rf_capacity;
    const int lane = (int)(threadIdx.x & 63u);
    const int wave = (int)(threadIdx.x >> 6);
    const int j = lane & (kOrGroup - 1);  // lane of the record's row
    const int grp = lane >> 4;
    const unsigned long long i = first + (threadIdx.x >> 4);

    // the record; one that does not name a sample of this geometry is dropped, never dereferenced
    bool active = i < n;
    uint4 rec0 = {0u, 0u, 0u, 0u}, rec1 = {0u, 0u, 0u, 0u};
    if (active) {
        rec0 = src[2 * i];
        rec1 = src[2 * i + 1];
    }
    const int o = (int)(rec0.x & 0xffffu);
    const int s = (int)((rec0.x >> 16) & 0xffu);
    const int r = (int)rec0.y, c = (int)rec0.z;
    active = active && o < g->O;
    int rows = 0, cols = 0;
    long long lev = 0;
    const float* P = pyr;
    if (active) {
        const OctGeom& og = g->oct[o];
        rows = og.rows;
        cols = og.cols;
        lev = og.lev_stride;
        P = pyr + (long long)b * g->pyr_stride + og.lev_off;
    }
    const int S = g->S;
    active = active && s >= 1 && s <= S && r >= 1 && r <= rows - 2 && c >= 1 && c <= cols - 2;
    const int R = active ? or_radius(s) : 0;
    const int nc = 2 * R + 3;  // rows and columns of L the record reads
    const int rr = r - R - 1 + j;
    const bool live = active && j < nc;

    // this lane's row of L = P[S+2] + P[S+1] + ... + P[s]; levels below s are never read
    float L[kOrCols];
#pragma unroll
    for (int q = 0; q < kOrCols; ++q) L[q] = 0.0f;
    if (live) {
        const float* const row = P + (long long)min(max(rr, 0), rows - 1) * cols;
        int cx[kOrCols];
#pragma unroll
        for (int q = 0; q < kOrCols; ++q) cx[q] = min(max(c - R - 1 + q, 0), cols - 1);
        const float* lv = row + (long long)(S + 2) * lev;
#pragma unroll
        for (int q = 0; q < kOrCols; ++q)
            if (q < nc) L[q] = lv[cx[q]];
        for (int t = S + 1; t >= s; --t) {
            lv -= lev;
            float x[kOrCols];
#pragma unroll
            for (int q = 0; q < kOrCols; ++q) x[q] = 0.0f;
#pragma unroll
            for (int q = 0; q < kOrCols; ++q)
                if (q < nc) x[q] = lv[cx[q]];
#pragma unroll
            for (int q = 0; q < kOrCols; ++q) L[q] = L[q] + x[q];
        }
    }
    // the rows above and below, from the neighbour lanes (every lane of the wave executes these)
    float up[kOrCols - 2], dn[kOrCols - 2];
#pragma unroll
    for (int q = 1; q < kOrCols - 1; ++q) {
        up[q - 1] = or_lane_up(L[q]);
        dn[q - 1] = or_lane_down(L[q]);
    }

    // the row's partial histogram, samples in ascending dc
    float* const mine = or_part[wave][lane];
#pragma unroll
    for (int k = 0; k < kOrBins; ++k) mine[k] = 0.0f;
    bool bad = false;
    if (live && j >= 1 && j <= 2 * R + 1 && rr >= 1 && rr <= rows - 2) {
        const int dr = j - R - 1;
        const float* const w = weights + (s - 1) * kOrWeights + dr * dr;
#pragma unroll
        for (int q = 1; q < kOrCols - 1; ++q) {
            const int dc = q - 1 - R;
            const int cc = c + dc;
            if (q <= 2 * R + 1 && cc >= 1 && cc <= cols - 2) {
                const float gx = L[q + 1] - L[q - 1];
                const float gy = dn[q - 1] - up[q - 1];
                const float m = sqrtf(gx * gx + gy * gy);
                if (!(m < INFINITY)) {
                    bad = true;  // NaN or inf: the whole record is rejected
                } else if (m > 0.0f) {
                    float* const p = mine + or_bin(gx, gy);
                    *p = *p + m * w[dc * dc];
                }
            }
        }
    }
    const bool reject = ((__ballot(bad) >> (16 * grp)) & 0xffffull) != 0;
    __builtin_amdgcn_wave_barrier();

    // hist[k] = the partials in ascending dr; lane j takes bins j, j + 16, j + 32.  Lanes that own no
    // sample row left their slice +0, and every term is >= +0, so adding it is the identity.
    float* const hist = or_hist[wave][grp][0];
    float* const smooth = or_hist[wave][grp][1];
#pragma unroll
    for (int t = 0; t < 3; ++t) {
        const int k = j + 16 * t;
        if (k < kOrBins) {
            float a = 0.0f;
#pragma unroll
            for (int d = 1; d <= 2 * kOrMaxR + 1; ++d)
                if (d <= 2 * R + 1) a = a + or_part[wave][16 * grp + d][k];
            hist[k] = a;
        }
    }
    __builtin_amdgcn_wave_barrier();
    float hk[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int t = 0; t < 3; ++t) {
        const int k = j + 16 * t;
        if (k < kOrBins) {
            const int m2 = k >= 2 ? k - 2 : k + 34, m1 = k >= 1 ? k - 1 : 35;
            const int p1 = k <= 34 ? k + 1 : 0, p2 = k <= 33 ? k + 2 : k - 34;
            hk[t] = ((hist[m2] + hist[p2]) * 0.0625f + (hist[m1] + hist[p1]) * 0.25f) + hist[k] * 0.375f;
            smooth[k] = hk[t];
        }
    }
    __builtin_amdgcn_wave_barrier();
    // every lane of the row reads the 36 smoothed bins: the maximum, and the finiteness test
    float mx = smooth[0];
    bool finite = fabsf(mx) < INFINITY;
#pragma unroll
    for (int k = 1; k < kOrBins; ++k) {
        const float v = smooth[k];
        finite = finite && fabsf(v) < INFINITY;
        if (v > mx) mx = v;
    }
    const float thr = mx * 0.8f;
    const bool ok = active && !reject && finite;
    bool hit[3];
    float angle[3];
    unsigned long long mask[3];
    unsigned total = 0, peaks = 0;
#pragma unroll
    for (int t = 0; t < 3; ++t) {
        const int k = j + 16 * t;
        hit[t] = false;
        angle[t] = 0.0f;
        if (ok && k < kOrBins) {
            const float l = smooth[k >= 1 ? k - 1 : 35], rt = smooth[k <= 34 ? k + 1 : 0];
            if (hk[t] > l && hk[t] > rt && hk[t] >= thr) {
                hit[t] = true;
                float bb = (float)k + (0.5f * (l - rt)) / ((l - 2.0f * hk[t]) + rt);
                if (bb < 0.0f) bb = bb + 36.0f;
                if (bb >= 36.0f) bb = bb - 36.0f;
                angle[t] = bb * 10.0f;
            }
        }
        mask[t] = __ballot(hit[t]);
        total += (unsigned)__popcll(mask[t]);
        peaks += (unsigned)__popcll((mask[t] >> (16 * grp)) & 0xffffull);
    }
    if (total == 0) return;  // wave-uniform
    unsigned base = 0;
    if (lane == 0) base = atomicAdd(count_out + b, total);
    base = (unsigned)__builtin_amdgcn_readfirstlane((int)base);
    uint4* const out = recs_out + 3ull * b * capacity;
#pragma unroll
    for (int t = 0; t < 3; ++t) {
        const unsigned rank =
            __builtin_amdgcn_mbcnt_hi((unsigned)(mask[t] >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask[t], 0u));
        const unsigned long long slot = (unsigned long long)base + rank;
        // the counter counts every record; nothing is stored at or beyond the capacity
        if (hit[t] && slot < capacity) {
            uint4* const p = out + 3ull * slot;
            p[0] = rec0;
            p[1] = rec1;
            p[2] = uint4{__float_as_uint(angle[t]), __float_as_uint(hk[t]), (unsigned)(j + 16 * t), peaks};
        }
        base += (unsigned)__popcll(mask[t]);
    }
}
