// gdp_describe.inc — SIFT descriptors of the oriented keypoints on the current pyramid: k_describe.
// Part of libgdp's single translation unit: included by gdp.hip inside its anonymous namespace
// (after `#pragma clang fp contract(off)`, which therefore applies here too).  Not a header.

// gdp_describe_keypoints (gdp.h): for every oriented record (o, s, r, c, angle) the Gaussian level
// L = P[S+2] + P[S+1] + ... + P[s] is rebuilt around the sample as k_orient does, the gradients of a
// (2R+1)^2 window are rotated by the record's angle (a host-built table of quarter degrees), split
// trilinearly over 4 x 4 spatial and 8 orientation bins and normalised into 128 bytes.  Every operation
// is the separately rounded float32 operation gdp.h writes down, in its order; the square roots and the
// divisions are IEEE-correct (sqrtf, plain `/`); no exp, sin, cos or atan2 runs here.
//
// One 32-lane half-wave per input record, two records per wave, one wave per block over batch x
// ceil(inputs / 2).  Lane q of a half first owns COLUMN c - R - 1 + q of the window (2R + 3 <= 25
// lanes live): it sums its column of L over the 2R + 3 rows in registers (addresses clamped into the
// level: a clamped value is only ever a neighbour of a sample the rule skips), so a row of the window
// is one contiguous read of the half, and writes it into the record's LDS tile.  Lane j then owns
// window ROW dr = j - R (2R + 1 <= 23 lanes live): it runs its samples in ascending dc, reading the
// three tile rows it needs, into its own 128-float LDS slice — the rule's per-row partial, no
// atomics.  The half adds the slices in ascending dr (lane j: bins j, j + 32, j + 64, j + 96), takes
// the two tree sums (their first two steps inside the lane, the last five across lanes), and stores
// the record with eleven 16-byte stores, compacted per wave as k_orient does (ballot + rank, one
// atomic per wave).  A record never spans waves and a wave's LDS operations complete in order: no
// block barrier.
constexpr int kDeBlock = 64;
constexpr int kDeGroup = 32;                             // lanes per record: half a wave
constexpr int kDePerBlock = kDeBlock / kDeGroup;         // records per block
constexpr int kDeBins = 128;                             // [4 row bins][4 col bins][8 orientation bins]
constexpr int kDeMaxR = 11;                              // radius of scale 1, the largest
constexpr int kDeCols = 2 * kDeMaxR + 3;                 // columns (and rows) of L a record reads at most
constexpr int kDeRows = 2 * kDeMaxR + 1;                 // window rows: lanes that own a slice at most
constexpr int kDeTile = (kDeCols * kDeCols + 3) / 4 * 4; // floats of a record's tile: whole 16-byte words
constexpr int kDeWeights = 2 * kDeMaxR * kDeMaxR + 1;    // W_s[d2], d2 = 0 .. 2 R^2: floats per scale
constexpr int kDeSlice = kDeBins + 1;                    // a lane's LDS slice; the odd pitch spreads the lanes' bins over the banks
constexpr int kDeAngles = 1440;                          // quarter-degree steps of the rotation table
constexpr unsigned kDeNoList = 0xffffffffu;              // own_count[b]: image b reads the orientation object's list
static_assert(sizeof(gdp_keypoint_described) == 176 && sizeof(gdp_keypoint_oriented) == 48, "eleven / three 16-byte words per record");
static_assert(kDeCols <= kDeGroup && kDeBins == 4 * kDeGroup, "a lane per window column, four bins per lane");
static_assert(kDePerBlock * (kDeTile + kDeRows * kDeSlice) * 4 <= 64 * 1024 && kDeTile * 4 >= kDeBins, "static LDS per block");

// round(3 sigma_s * sqrt(2) * 2.5), sigma_s = 2 / (s + 1): 11, 7, 5, 4, 4, 3, 3, 2, 2, ...
__host__ __device__ __forceinline__ int de_radius(int s) { return (2121 + 50 * (s + 1)) / (100 * (s + 1)); }

// A(t) ~ atan(t) * 4 / pi on [0, 1]: gdp.h's odd polynomial, Horner form, every step rounded
__device__ __forceinline__ float de_octant(float t) {
    constexpr unsigned C[6] = {0x3fa2f890u, 0xbed8d61du, 0x3e7c5661u, 0xbe17cbe9u, 0x3d89486eu, 0xbc74784eu};
    const float z = t * t;
    float p = __uint_as_float(C[5]);
#pragma unroll
    for (int k = 4; k >= 0; --k) p = p * z + __uint_as_float(C[k]);
    return p * t;
}

// the orientation of (gu, gv) in bins of 45 degrees, [0, 8): the quadrant as k_orient takes it, then
// the polynomial on the smaller over the larger component
__device__ __forceinline__ float de_orientation(float gu, float gv) {
    int q;
    float ax, ay;
    if (gu > 0.0f && gv >= 0.0f) {
        q = 0, ax = gu, ay = gv;
    } else if (gu <= 0.0f && gv > 0.0f) {
        q = 1, ax = gv, ay = -gu;
    } else if (gu < 0.0f && gv <= 0.0f) {
        q = 2, ax = -gu, ay = -gv;
    } else {
        q = 3, ax = -gv, ay = gu;
    }
    float w8;
    if (ay <= ax)
        w8 = ax > 0.0f ? de_octant(ay / ax) : 0.0f;
    else
        w8 = 2.0f - de_octant(ax / ay);
    float ob = (float)(2 * q) + w8;
    if (ob >= 8.0f) ob = ob - 8.0f;
    return ob;
}

// t[i] = t[i] + t[i + step] for step = 16 .. 1 within the half-wave, then t[0] to every lane: the last
// five steps of gdp.h's tree (lanes at or above `step` compute values nobody reads)
__device__ __forceinline__ float de_tree(float t) {
#pragma unroll
    for (int step = 16; step >= 1; step >>= 1) t = t + __shfl_down(t, step, kDeGroup);
    return __shfl(t, 0, kDeGroup);
}

__global__ void __launch_bounds__(kDeBlock) k_describe(const Geom* __restrict__ g, const float* __restrict__ pyr,
                                                       const uint4* __restrict__ orr, const unsigned* __restrict__ orr_count,
                                                       unsigned long long orr_capacity, const uint4* __restrict__ own,
                                                       const unsigned* __restrict__ own_count,
                                                       const float* __restrict__ weights, const float* __restrict__ rot,
                                                       uint4* __restrict__ recs_out, unsigned* __restrict__ count_out,
                                                       unsigned long long capacity, unsigned blocks_per_img) {
    __shared__ __attribute__((aligned(16))) float de_tile[kDePerBlock][kDeTile];  // per record: L around the sample, [row][column]
    __shared__ float de_part[kDePerBlock][kDeRows][kDeSlice];   // per window row: its partial histogram
    const unsigned b = blockIdx.x / blocks_per_img;
    const unsigned long long first = (unsigned long long)(blockIdx.x - b * blocks_per_img) * kDePerBlock;
    // the list: the caller's (gdp_describe_set_input) or the orientation object's; block-uniform.  An
    // image with neither (no orientation object) reads an empty one: orr_capacity is 0
    const unsigned n_own = own_count[b];
    const unsigned long long n =
        n_own != kDeNoList ? (unsigned long long)n_own : (orr_capacity ? min((unsigned long long)orr_count[b], orr_capacity) : 0ull);
    if (first >= n) return;
    const uint4* const src = n_own != kDeNoList ? own + 3ull * b * capacity : orr + 3ull * b * orr_capacity;
    const int lane = (int)(threadIdx.x & 63u);
    const int j = lane & (kDeGroup - 1);  // lane of the record's half
    const int grp = lane >> 5;
    const unsigned long long i = first + (unsigned)grp;

    // the record; one that does not name a sample of this geometry, or whose angle is outside
    // [0, 360), is dropped, never dereferenced
    bool active = i < n;
    uint4 rec0 = {0u, 0u, 0u, 0u}, rec1 = {0u, 0u, 0u, 0u}, rec2 = {0u, 0u, 0u, 0u};
    if (active) {
        rec0 = src[3 * i];
        rec1 = src[3 * i + 1];
        rec2 = src[3 * i + 2];
    }
    const int o = (int)(rec0.x & 0xffffu);
    const int s = (int)((rec0.x >> 16) & 0xffu);
    const int r = (int)rec0.y, c = (int)rec0.z;
    const float angle = __uint_as_float(rec2.x);
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
    active = active && s >= 1 && s <= S && r >= 1 && r <= rows - 2 && c >= 1 && c <= cols - 2 && 0.0f <= angle && angle < 360.0f;
    const int R = active ? de_radius(s) : 0;
    const int nc = 2 * R + 3;  // rows and columns of L the record reads

    // this lane's column of L = P[S+2] + P[S+1] + ... + P[s]; levels below s are never read
    float* const tile = de_tile[grp];
    if (active && j < nc) {
        const float* lv = P + (long long)(S + 2) * lev + min(max(c - R - 1 + j, 0), cols - 1);
        long long ro[kDeCols];
#pragma unroll
        for (int q = 0; q < kDeCols; ++q) ro[q] = (long long)min(max(r - R - 1 + q, 0), rows - 1) * cols;
        float L[kDeCols];
#pragma unroll
        for (int q = 0; q < kDeCols; ++q) L[q] = q < nc ? lv[ro[q]] : 0.0f;
        for (int t = S + 1; t >= s; --t) {
            lv -= lev;
            float x[kDeCols];
#pragma unroll
            for (int q = 0; q < kDeCols; ++q) x[q] = q < nc ? lv[ro[q]] : 0.0f;
#pragma unroll
            for (int q = 0; q < kDeCols; ++q) L[q] = L[q] + x[q];
        }
#pragma unroll
        for (int q = 0; q < kDeCols; ++q)
            if (q < nc) tile[q * kDeCols + j] = L[q];
    }
    // the partials of the window's rows start at +0
    float* const part = &de_part[grp][0][0];
    for (int k = j; k < (2 * R + 1) * kDeSlice; k += kDeGroup) part[k] = 0.0f;
    __builtin_amdgcn_wave_barrier();

    // the rotation, and this lane's window row: its samples in ascending dc
    bool bad = false;
    const int dr = j - R;
    if (active && j <= 2 * R && r + dr >= 1 && r + dr <= rows - 2) {
        int a = (int)(angle * 4.0f + 0.5f);
        if (a >= kDeAngles) a -= kDeAngles;
        const float ca = rot[a], sa = rot[kDeAngles + a];
        const float inv_s = (float)(s + 1) / 6.0f;
        const float* const w = weights + (s - 1) * kDeWeights + dr * dr;
        const float y = (float)dr;
        float* const mine = part + j * kDeSlice;
        const float* const mid = tile + (j + 1) * kDeCols + R + 1;  // L[r + dr][c]
        for (int dc = -R; dc <= R; ++dc) {
            const int cc = c + dc;
            if (cc < 1 || cc > cols - 2) continue;
            const float x = (float)dc;
            const float cb = ((x * ca + y * sa) * inv_s) + 1.5f;
            const float rb = ((y * ca - x * sa) * inv_s) + 1.5f;
            if (!(rb > -1.0f && rb < 4.0f && cb > -1.0f && cb < 4.0f)) continue;
            const float gx = mid[dc + 1] - mid[dc - 1];
            const float gy = mid[dc + kDeCols] - mid[dc - kDeCols];
            const float m = sqrtf(gx * gx + gy * gy);
            if (!(m < INFINITY)) {
                bad = true;  // NaN or inf: the whole record is rejected
                continue;
            }
            if (!(m > 0.0f)) continue;
            const float gu = gx * ca + gy * sa;
            const float gv = gy * ca - gx * sa;
            const float ob = de_orientation(gu, gv);
            const float r0 = floorf(rb), c0 = floorf(cb), o0 = floorf(ob);
            const float fr = rb - r0, fc = cb - c0, fo = ob - o0;
            const float mag = m * w[dc * dc];
            const int ir = (int)r0, ic = (int)c0, io = (int)o0;
            const float v1 = mag * fr, v0 = mag - v1;
#pragma unroll
            for (int a1 = 0; a1 < 2; ++a1) {
                const float v = a1 ? v1 : v0;
                const float vc1 = v * fc, vc0 = v - vc1;
#pragma unroll
                for (int a2 = 0; a2 < 2; ++a2) {
                    const float vc = a2 ? vc1 : vc0;
                    const float vo1 = vc * fo, vo0 = vc - vo1;
                    const int br = ir + a1, bc = ic + a2;
                    if (br >= 0 && br <= 3 && bc >= 0 && bc <= 3) {
                        float* const p = mine + (br * 4 + bc) * 8;
                        const int k0 = io & 7, k1 = (io + 1) & 7;
                        p[k0] = p[k0] + vo0;
                        p[k1] = p[k1] + vo1;
                    }
                }
            }
        }
    }
    const bool reject = ((__ballot(bad) >> (kDeGroup * grp)) & 0xffffffffull) != 0;
    __builtin_amdgcn_wave_barrier();

    // hist[k] = the partials in ascending dr; lane j takes bins j, j + 32, j + 64, j + 96.  A row the
    // rule skips left its slice +0, and every term is >= +0, so adding it is the identity.
    float h[4];
    bool finite = true;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        float acc = 0.0f;
        for (int d = 0; d <= 2 * R; ++d) acc = acc + part[d * kDeSlice + j + kDeGroup * t];
        h[t] = acc;
        finite = finite && acc < INFINITY;
    }
    const bool overflow = ((__ballot(!finite) >> (kDeGroup * grp)) & 0xffffffffull) != 0;
    // T(hist): steps 64 and 32 of the tree pair this lane's own four bins
    const float n1 = sqrtf(de_tree((h[0] * h[0] + h[2] * h[2]) + (h[1] * h[1] + h[3] * h[3])));
    const bool ok = active && !reject && !overflow && n1 > 0.0f && n1 < INFINITY;
    const float div = ok ? n1 : 1.0f;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        h[t] = h[t] / div;
        if (h[t] > 0.2f) h[t] = 0.2f;
    }
    const float n2 = sqrtf(de_tree((h[0] * h[0] + h[2] * h[2]) + (h[1] * h[1] + h[3] * h[3])));
    const float div2 = ok ? n2 : 1.0f;
    // the bytes go through the record's tile (its values are used up) so that a lane stores 16 of them
    __builtin_amdgcn_wave_barrier();
    unsigned char* const bytes = reinterpret_cast<unsigned char*>(tile);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const float qv = (h[t] / div2) * 512.0f;
        bytes[j + kDeGroup * t] = qv >= 255.0f ? (unsigned char)255 : (unsigned char)(int)qv;
    }
    __builtin_amdgcn_wave_barrier();

    // one slot per kept record: the wave's two halves, ranked by half
    const unsigned long long kept = __ballot(ok && j == 0);
    if (kept == 0) return;  // wave-uniform
    unsigned base = 0;
    if (lane == 0) base = atomicAdd(count_out + b, (unsigned)__popcll(kept));
    base = (unsigned)__builtin_amdgcn_readfirstlane((int)base);
    const unsigned long long slot = (unsigned long long)base + (unsigned)(grp == 1 && (kept & 1ull) ? 1 : 0);
    // the counter counts every record; nothing is stored at or beyond the capacity
    if (ok && slot < capacity && j < 11) {
        uint4 word;
        if (j == 0)
            word = rec0;
        else if (j == 1)
            word = rec1;
        else if (j == 2)
            word = rec2;
        else
            word = reinterpret_cast<const uint4*>(tile)[j - 3];
        recs_out[11ull * ((unsigned long long)b * capacity + slot) + (unsigned)j] = word;
    }
}
