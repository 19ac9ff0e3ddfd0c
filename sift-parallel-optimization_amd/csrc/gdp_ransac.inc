// RANSAC homography of a match list (extension; the rule is in include/gdp.h): H hypotheses, each the
// exact four-point homography of four sampled matches, scored against every match; the best one's
// inliers are the result.
//
// k_ransac_fit      one thread per hypothesis: the sample (integers), the homography in FP64 without
//                   a division, normalised and rounded to float32; stores the 64-byte record
// k_ransac_score    the hot path.  lane = hypothesis (its nine floats in VGPRs), the matches are
//                   wave-uniform (scalar loads of the four coordinates), the count lives in a register:
//                   no cross-lane work per pair, one integer atomicAdd per lane and match chunk
// k_ransac_select   one block: the maximum of (count, lowest index) over the H counts; the model record
// k_ransac_inliers  one thread per match: the test again under the model, compacted per wave
//
// Every float operation of the rule is written as one C++ operation; the library is built with
// -ffp-contract=off -fno-fast-math -fno-gpu-flush-denormals-to-zero, which is part of the rule.

constexpr int kRaHypTile = 256;        // hypotheses (threads) per block of k_ransac_score and k_ransac_fit
constexpr int kRaMatchTile = 64;       // a chunk of the match list is a multiple of this many records
constexpr int kRaGroup = 8;            // matches whose scalar loads are issued together
constexpr int kRaTargetWaves = 8192;   // chunks are added until the capacity grid has this many waves
constexpr uint32_t kRaMaxHypotheses = 65536, kRaDefaultHypotheses = 4096;

// The list a fit reads: the caller's, else the match object's output (gdp_pairs.inc); its own type as MaSide is
struct RaList : ListRef<const uint4*> {};

__device__ __forceinline__ uint32_t ra_mix(uint32_t x) {
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}

// adj(M) in the header's order: nine times two rounded products and one rounded difference
__device__ __forceinline__ void ra_adj(const double (&M)[3][3], double (&J)[3][3]) {
    J[0][0] = M[1][1] * M[2][2] - M[1][2] * M[2][1];
    J[0][1] = M[0][2] * M[2][1] - M[0][1] * M[2][2];
    J[0][2] = M[0][1] * M[1][2] - M[0][2] * M[1][1];
    J[1][0] = M[1][2] * M[2][0] - M[1][0] * M[2][2];
    J[1][1] = M[0][0] * M[2][2] - M[0][2] * M[2][0];
    J[1][2] = M[0][2] * M[1][0] - M[0][0] * M[1][2];
    J[2][0] = M[1][0] * M[2][1] - M[1][1] * M[2][0];
    J[2][1] = M[0][1] * M[2][0] - M[0][0] * M[2][1];
    J[2][2] = M[0][0] * M[1][1] - M[0][1] * M[1][0];
}

// step 2: the matrix taking the projective basis to the four points (x[k], y[k])
__device__ __forceinline__ void ra_basis(const double (&x)[4], const double (&y)[4], double (&A)[3][3]) {
    double M[3][3], J[3][3], lam[3];
    for (int c = 0; c < 3; ++c) {
        M[0][c] = x[c];
        M[1][c] = y[c];
        M[2][c] = 1.0;
    }
    ra_adj(M, J);
    for (int r = 0; r < 3; ++r) lam[r] = (J[r][0] * x[3] + J[r][1] * y[3]) + J[r][2];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) A[r][c] = M[r][c] * lam[c];
}

// step 5 for one pair: the same expression in k_ransac_score and k_ransac_inliers
__device__ __forceinline__ bool ra_inlier(const float (&h)[9], float x, float y, float X, float Y, float tt) {
    float u, v, w;
    project(h, x, y, u, v, w);
    const float dx = X * w - u;
    const float dy = Y * w - v;
    const float e = dx * dx + dy * dy;
    const bool front = w > 0.0f, near = e <= tt * (w * w);
    return front & near;  // both evaluated: no branch per pair
}

// One thread per hypothesis; the grid is sized from H.  hyp[h] = the whole record, count 0.
__global__ __launch_bounds__(kRaHypTile) void k_ransac_fit(RaList L, uint32_t H, uint32_t seed, uint4* __restrict__ hyp) {
    const uint32_t h = blockIdx.x * (uint32_t)kRaHypTile + threadIdx.x;
    if (h >= H) return;
    const uint4* recs;
    const unsigned n = list_resolve(L, recs);
    uint32_t idx[4];
    for (uint32_t k = 0; k < 4; ++k) idx[k] = __umulhi(ra_mix(seed + 0x9e3779b9u * (4u * h + k + 1u)), n);
    bool valid = n >= 4 && idx[0] != idx[1] && idx[0] != idx[2] && idx[0] != idx[3] && idx[1] != idx[2] && idx[1] != idx[3] &&
                 idx[2] != idx[3];
    float hf[9] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (valid) {  // idx[k] < n: (r * n) >> 32 with r < 2^32
        double qx[4], qy[4], tx[4], ty[4];
        for (int k = 0; k < 4; ++k) {
            const uint4 c = recs[2 * (size_t)idx[k] + 1];  // qx, qy, tx, ty
            qx[k] = (double)__uint_as_float(c.x);
            qy[k] = (double)__uint_as_float(c.y);
            tx[k] = (double)__uint_as_float(c.z);
            ty[k] = (double)__uint_as_float(c.w);
        }
        double A[3][3], B[3][3], J[3][3], G[3][3];
        ra_basis(qx, qy, A);
        ra_basis(tx, ty, B);
        ra_adj(A, J);
        double s = 0.0;
        bool nan = false;
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) {
                const double g = (B[r][0] * J[0][c] + B[r][1] * J[1][c]) + B[r][2] * J[2][c];
                G[r][c] = g;
                const double a = fabs(g);
                nan = nan || g != g;
                s = a > s ? a : s;  // a NaN never becomes s: `nan` remembers it
            }
        valid = !nan && s > 0.0 && s < __builtin_inf();
        if (valid) {
            int e;
            (void)frexp(s, &e);
            for (int r = 0; r < 3; ++r)
                for (int c = 0; c < 3; ++c) G[r][c] = ldexp(G[r][c], -e);
            const double w0 = (G[2][0] * qx[0] + G[2][1] * qy[0]) + G[2][2];
            const bool flip = w0 < 0.0;
            for (int r = 0; r < 3; ++r)
                for (int c = 0; c < 3; ++c) hf[3 * r + c] = (float)(flip ? -G[r][c] : G[r][c]);
        }
    }
    uint4* out = hyp + 4 * (size_t)h;
    out[0] = make_uint4(__float_as_uint(hf[0]), __float_as_uint(hf[1]), __float_as_uint(hf[2]), __float_as_uint(hf[3]));
    out[1] = make_uint4(__float_as_uint(hf[4]), __float_as_uint(hf[5]), __float_as_uint(hf[6]), __float_as_uint(hf[7]));
    out[2] = make_uint4(__float_as_uint(hf[8]), h, 0u, n);  // h[8], hypothesis, inliers, matches
    out[3] = make_uint4(idx[0], idx[1], idx[2], idx[3]);
}

// blockIdx.x: kRaHypTile hypotheses, blockIdx.y: chunk of the match list.  Both grid dimensions are
// sized from the capacities; the chunk length comes from the count read here.  hyp[h].inliers (word
// 10 of the record) += this chunk's count.
__global__ __launch_bounds__(kRaHypTile) void k_ransac_score(RaList L, uint32_t H, float tt, unsigned chunks,
                                                              uint32_t* __restrict__ hyp) {
    const uint32_t first = blockIdx.x * (uint32_t)kRaHypTile + (threadIdx.x & ~63u);
    if (first >= H) return;  // wave-uniform
    const uint4* recs;
    const unsigned n = list_resolve(L, recs);
    const unsigned len = chunk_len(n, chunks, kRaMatchTile);
    const unsigned long long begin64 = (unsigned long long)blockIdx.y * len;
    if (begin64 >= n) return;  // covers n == 0
    const unsigned begin = (unsigned)begin64, end = n - begin < len ? n : begin + len;
    const uint32_t h = blockIdx.x * (uint32_t)kRaHypTile + threadIdx.x;
    const uint32_t hc = h < H ? h : H - 1;  // clamped; a masked lane's count is never added
    float m[9];
    {
        const uint4* p = reinterpret_cast<const uint4*>(hyp) + 4 * (size_t)hc;
        const uint4 a = p[0], b = p[1];
        m[0] = __uint_as_float(a.x), m[1] = __uint_as_float(a.y), m[2] = __uint_as_float(a.z), m[3] = __uint_as_float(a.w);
        m[4] = __uint_as_float(b.x), m[5] = __uint_as_float(b.y), m[6] = __uint_as_float(b.z), m[7] = __uint_as_float(b.w);
        m[8] = __uint_as_float(hyp[16 * (size_t)hc + 8]);
    }
    // the coordinates are the second 16 bytes of a record; the address is the same in every lane
    const uint4* __restrict__ xy = recs + 1;
    uint32_t count = 0;
    unsigned i = begin;
    for (; i + kRaGroup <= end; i += kRaGroup) {
        uint4 c[kRaGroup];
        for (int k = 0; k < kRaGroup; ++k) c[k] = xy[2 * (size_t)(i + k)];
        for (int k = 0; k < kRaGroup; ++k)
            count += ra_inlier(m, __uint_as_float(c[k].x), __uint_as_float(c[k].y), __uint_as_float(c[k].z), __uint_as_float(c[k].w), tt)
                         ? 1u
                         : 0u;
    }
    for (; i < end; ++i) {
        const uint4 c = xy[2 * (size_t)i];
        count += ra_inlier(m, __uint_as_float(c.x), __uint_as_float(c.y), __uint_as_float(c.z), __uint_as_float(c.w), tt) ? 1u : 0u;
    }
    if (h < H && count != 0) atomicAdd(hyp + 16 * (size_t)h + 10, count);
}

// One block.  The winner maximises (count, lowest h): as one word, (count << 32) | ~h.  model = its
// record when count >= max(min_inliers, 4), else the "none" record.  A hypothesis that counted 4 or
// more is a valid one (an invalid one has h[] = 0, so w = 0 and it counts nothing).
__global__ __launch_bounds__(1024) void k_ransac_select(RaList L, uint32_t H, uint32_t min_inliers, const uint4* __restrict__ hyp,
                                                        uint4* __restrict__ model) {
    __shared__ unsigned long long best[16];
    unsigned long long key = 0;
    for (uint32_t h = threadIdx.x; h < H; h += 1024u) {
        const unsigned long long k = ((unsigned long long)hyp[4 * (size_t)h + 2].z << 32) | (uint32_t)~h;
        key = k > key ? k : key;
    }
    for (int d = 32; d >= 1; d >>= 1) {
        const unsigned long long o = (unsigned long long)__shfl_xor((long long)key, d);
        key = o > key ? o : key;
    }
    if ((threadIdx.x & 63u) == 0) best[threadIdx.x >> 6] = key;
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int w = 1; w < 16; ++w) key = best[w] > key ? best[w] : key;
    const uint32_t count = (uint32_t)(key >> 32), win = ~(uint32_t)key;
    const uint32_t need = min_inliers > 4u ? min_inliers : 4u;
    if (count >= need) {  // count >= 4 > 0: the key came from a record, so win < H
        for (int k = 0; k < 4; ++k) model[k] = hyp[4 * (size_t)win + k];
        return;
    }
    const uint4* recs;
    const unsigned n = list_resolve(L, recs);
    model[0] = model[1] = make_uint4(0u, 0u, 0u, 0u);
    model[2] = make_uint4(0u, kNone, 0u, n);
    model[3] = make_uint4(kNone, kNone, kNone, kNone);
}

// One thread per match; the grid is sized from the capacity.  Writes nothing without a model.
__global__ __launch_bounds__(256) void k_ransac_inliers(RaList L, float tt, const uint4* __restrict__ model, uint4* __restrict__ out,
                                                        uint32_t* __restrict__ out_count) {
    const uint4* recs;
    const unsigned n = list_resolve(L, recs);
    const unsigned first = blockIdx.x * 256u + (threadIdx.x & ~63u);
    if (first >= n) return;  // wave-uniform
    const uint32_t* words = reinterpret_cast<const uint32_t*>(model);
    if (words[9] == kNone) return;  // the record's `hypothesis`
    float m[9];
    load_model(words, nullptr, m);
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    bool keep = i < n;
    uint4 lo = make_uint4(0, 0, 0, 0), hi = lo;
    if (keep) {
        lo = recs[2 * (size_t)i];
        hi = recs[2 * (size_t)i + 1];
        keep = ra_inlier(m, __uint_as_float(hi.x), __uint_as_float(hi.y), __uint_as_float(hi.z), __uint_as_float(hi.w), tt);
    }
    emit_match_record(keep, lo, hi, out, out_count);  // at most n <= the capacity records
}
