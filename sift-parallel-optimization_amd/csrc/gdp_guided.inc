// Guided matching under a homography (extension; the rule is in include/gdp.h): every query is projected
// into the train frame and matched against the train records inside a square window round its
// projection only.  The train records are binned into a uniform grid (a cell list) over the train
// frame, and a query visits the cells its window touches.
//
//   cell(x) = clamp(floorf(x * (1 / c)), 0, G - 1),  c a power of two
//
// is monotone non-decreasing in x (the rounded product, floorf and the clamp each are), so every train
// with x0 <= tx <= x1 lies in a cell of cell(x0) .. cell(x1): the cell search visits a superset of the
// rule's candidates and the four comparisons of the rule decide, whatever the float arithmetic rounds.
//
// k_guided_prepare  blockIdx.y = 0: one thread per query: coordinates, projection, window, sum d^2
//                   blockIdx.y = 1: one thread per train: coordinates, sum d^2, its cell, the histogram
//                   of trains per cell, and its slot of the per-train minimum set to "none"
// k_guided_scan     one block: the exclusive scan of the histogram (start[], and the cursors in place)
// k_guided_scatter  one thread per train: (tx, ty, sum d^2, j) into cell order.  Cells are row-major, so
//                   the cells of one window row are one contiguous range of the ordered array.  The
//                   descriptors are NOT copied into that order: a launch would read and write every
//                   train descriptor once to save the few candidates' scattered 128-byte lines
// k_guided_search   the hot path.  Eight lanes per query: a lane keeps 16 bytes of the query descriptor
//                   and loads 16 bytes of each candidate, so the group reads a candidate as one 128-byte
//                   line; four v_dot4_u32_u8 per lane, three cross-lane steps inside the group
// k_guided_claim    (unique only) one thread per query: 64-bit atomicMin of (distance << 32) | query on
//                   its train's slot.  The minimum is commutative: no dependence on timing
// k_guided_select   one thread per query: ratio, cap, the unique test, compaction per wave
//
// dist = sum q^2 + sum t^2 - 2 sum q t on the unsigned bytes: 128 * 255^2 < 2^24, exact in uint32.

constexpr int kGuLanes = 8;                   // lanes per query of k_guided_search
constexpr int kGuBlock = 256;                 // its block: 32 queries
constexpr int kGuScanThreads = 1024;          // k_guided_scan's one block
constexpr uint32_t kGuDefaultCells = 1u << 18;  // cells of the grid at most, unless the caller says otherwise
constexpr uint32_t kGuMaxCells = 1u << 24;
constexpr int kGuMaxLog2Side = 64;            // the cell side is 2^0 .. 2^64

struct GuidedGrid {
    float inv_side;      // 1 / c, a power of two
    float xmax, ymax;    // (float)(Gx - 1), (float)(Gy - 1)
    unsigned gx, cells;  // cells per row; gx * gy
};

// sum d^2 on the unsigned bytes (k_match_norm's is of the bytes shifted by 128, for the MFMA path)
__device__ __forceinline__ uint32_t gu_norm(const char* rec) {
    const uint4* d = reinterpret_cast<const uint4*>(rec + kMaDesc);
    uint32_t sum = 0;
    for (int k = 0; k < 8; ++k) {
        const uint4 v = d[k];
        sum = __builtin_amdgcn_udot4(v.x, v.x, sum, false);
        sum = __builtin_amdgcn_udot4(v.y, v.y, sum, false);
        sum = __builtin_amdgcn_udot4(v.z, v.z, sum, false);
        sum = __builtin_amdgcn_udot4(v.w, v.w, sum, false);
    }
    return sum;
}

// the cell of a coordinate that is not a NaN: clamped in float, then converted
__device__ __forceinline__ unsigned gu_cell(float x, float inv_side, float cmax) {
    float f = floorf(x * inv_side);
    f = f < 0.0f ? 0.0f : f;
    f = f > cmax ? cmax : f;
    return (unsigned)f;
}

// `own` non-NULL: the caller's nine floats; else the fit's model record (all 0 when it holds no model).
__global__ __launch_bounds__(256) void k_guided_prepare(MaSide Q, MaSide T, const uint32_t* __restrict__ model,
                                                        const float* __restrict__ own, float radius, GuidedGrid g,
                                                        float4* __restrict__ win, float2* __restrict__ qxy, uint32_t* __restrict__ qnorm,
                                                        float2* __restrict__ txy, uint32_t* __restrict__ tnorm,
                                                        uint32_t* __restrict__ tcell, uint32_t* __restrict__ hist,
                                                        unsigned long long* __restrict__ tmin) {
    const unsigned k = blockIdx.x * 256u + threadIdx.x;
    const char* recs;
    if (blockIdx.y == 0) {
        const unsigned nq = list_resolve(Q, recs);
        if (k >= nq) return;
        const char* rec = recs + (size_t)k * kMaRecord;
        float h[9];
        load_model(model, own, h);
        float qx, qy, u, v, w;
        record_xy(rec, qx, qy);
        project(h, qx, qy, u, v, w);
        const float nan = __uint_as_float(0x7fc00000u);
        float4 box = make_float4(nan, nan, nan, nan);  // no window: every comparison fails
        if (w > 0.0f) {
            const float sx = u / w, sy = v / w;
            box = make_float4(sx - radius, sx + radius, sy - radius, sy + radius);
        }
        win[k] = box;
        qxy[k] = make_float2(qx, qy);
        qnorm[k] = gu_norm(rec);
        return;
    }
    const unsigned nt = list_resolve(T, recs);
    if (k >= nt) return;
    const char* rec = recs + (size_t)k * kMaRecord;
    float tx, ty;
    record_xy(rec, tx, ty);
    txy[k] = make_float2(tx, ty);
    tnorm[k] = gu_norm(rec);
    tmin[k] = ~0ull;
    uint32_t cell = kNone;  // a NaN coordinate is nobody's candidate: in no cell
    if (tx == tx && ty == ty) {
        cell = gu_cell(ty, g.inv_side, g.ymax) * g.gx + gu_cell(tx, g.inv_side, g.xmax);
        atomicAdd(hist + cell, 1u);
    }
    tcell[k] = cell;
}

// One block.  start[c] = trains in the cells below c, start[cells] = trains in a cell; hist[c] becomes
// start[c], the cursor k_guided_scatter counts up.
__global__ __launch_bounds__(kGuScanThreads) void k_guided_scan(uint32_t* __restrict__ hist, uint32_t* __restrict__ start,
                                                                 unsigned cells) {
    __shared__ uint32_t wave_sum[kGuScanThreads / 64];
    const unsigned tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const unsigned per = (cells + kGuScanThreads - 1) / kGuScanThreads;
    const unsigned long long b64 = (unsigned long long)tid * per;
    const unsigned begin = b64 < cells ? (unsigned)b64 : cells, end = cells - begin < per ? cells : begin + per;
    uint32_t sum = 0;
    for (unsigned c = begin; c < end; ++c) sum += hist[c];
    uint32_t incl = sum;
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t up = (uint32_t)__shfl_up((int)incl, d);
        if (lane >= (unsigned)d) incl += up;
    }
    if (lane == 63) wave_sum[wave] = incl;
    __syncthreads();
    uint32_t run = incl - sum;
    for (unsigned w = 0; w < wave; ++w) run += wave_sum[w];
    for (unsigned c = begin; c < end; ++c) {
        const uint32_t n = hist[c];
        start[c] = run;
        hist[c] = run;
        run += n;
    }
    if (tid == kGuScanThreads - 1) start[cells] = run;  // the last thread's range ends the grid
}

__global__ __launch_bounds__(256) void k_guided_scatter(MaSide T, const float2* __restrict__ txy, const uint32_t* __restrict__ tnorm,
                                                        const uint32_t* __restrict__ tcell, uint32_t* __restrict__ cursor,
                                                        uint4* __restrict__ ordered) {
    const char* recs;
    const unsigned nt = list_resolve(T, recs);
    const unsigned j = blockIdx.x * 256u + threadIdx.x;
    if (j >= nt) return;
    const uint32_t cell = tcell[j];
    if (cell == kNone) return;
    const uint32_t at = atomicAdd(cursor + cell, 1u);  // below start[cell + 1] <= nt: the histogram counted this train
    const float2 p = txy[j];
    ordered[at] = make_uint4(__float_as_uint(p.x), __float_as_uint(p.y), tnorm[j], j);
}

// Query blockIdx.x * 32 + threadIdx.x / 8.  best[i] = (distance, train, second, 0), all kNone without a candidate.
__global__ __launch_bounds__(kGuBlock) void k_guided_search(MaSide Q, MaSide T, GuidedGrid g, const float4* __restrict__ win,
                                                            const uint32_t* __restrict__ qnorm, const uint32_t* __restrict__ start,
                                                            const uint4* __restrict__ ordered, uint4* __restrict__ best) {
    const char *qrecs, *trecs;
    const unsigned nq = list_resolve(Q, qrecs);
    (void)list_resolve(T, trecs);
    const unsigned sub = threadIdx.x & (kGuLanes - 1);
    const unsigned i = blockIdx.x * (kGuBlock / kGuLanes) + threadIdx.x / kGuLanes;
    if (i >= nq) return;  // uniform in the group of eight lanes
    const uint4 qd = *reinterpret_cast<const uint4*>(qrecs + (size_t)i * kMaRecord + kMaDesc + 16u * sub);
    const uint32_t qn = qnorm[i];
    const float4 box = win[i];  // x0, x1, y0, y1
    uint32_t B = kNone, I = kNone, S = kNone;
    if (box.x <= box.y && box.z <= box.w) {  // false for a NaN: such a window has no candidate
        const unsigned cx0 = gu_cell(box.x, g.inv_side, g.xmax), cx1 = gu_cell(box.y, g.inv_side, g.xmax);
        const unsigned cy0 = gu_cell(box.z, g.inv_side, g.ymax), cy1 = gu_cell(box.w, g.inv_side, g.ymax);
        for (unsigned cy = cy0; cy <= cy1; ++cy) {
            const unsigned row = cy * g.gx;
            const uint32_t p_end = start[row + cx1 + 1];
            for (uint32_t p = start[row + cx0]; p < p_end; ++p) {
                const uint4 t = ordered[p];  // the same address in the eight lanes
                const float tx = __uint_as_float(t.x), ty = __uint_as_float(t.y);
                if (!(box.x <= tx && tx <= box.y && box.z <= ty && ty <= box.w)) continue;  // the rule's four comparisons
                const uint4 td = *reinterpret_cast<const uint4*>(trecs + (size_t)t.w * kMaRecord + kMaDesc + 16u * sub);
                uint32_t dot = __builtin_amdgcn_udot4(qd.x, td.x, 0u, false);
                dot = __builtin_amdgcn_udot4(qd.y, td.y, dot, false);
                dot = __builtin_amdgcn_udot4(qd.z, td.z, dot, false);
                dot = __builtin_amdgcn_udot4(qd.w, td.w, dot, false);
                // the group's sum in every lane of it: the quad's pairs, the quad, then the other quad of the eight
                dot += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)dot, 0xB1, 0xf, 0xf, true);   // quad_perm [1, 0, 3, 2]
                dot += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)dot, 0x4E, 0xf, 0xf, true);   // quad_perm [2, 3, 0, 1]
                dot += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)dot, 0x141, 0xf, 0xf, true);  // row_half_mirror: lane k <-> 7 - k
                const uint32_t d = qn + t.z - 2u * dot;
                if (d < B || (d == B && t.w < I)) {  // (distance, index) lexicographic: the order in a cell does not matter
                    S = B;
                    B = d;
                    I = t.w;
                } else {
                    S = S < d ? S : d;
                }
            }
        }
    }
    if (sub == 0) best[i] = make_uint4(B, I, S, 0u);
}

__global__ __launch_bounds__(256) void k_guided_claim(MaSide Q, const uint4* __restrict__ best, int use_ratio, float r2,
                                                      uint32_t max_distance, unsigned long long* __restrict__ tmin) {
    const char* recs;
    const unsigned nq = list_resolve(Q, recs);
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= nq) return;
    const uint4 b = best[i];
    if (passes_ratio_and_cap(b.x, b.y, b.z, use_ratio, r2, max_distance)) atomicMin(tmin + b.y, ((unsigned long long)b.x << 32) | i);  // b.y < nt
}

__global__ __launch_bounds__(256) void k_guided_select(MaSide Q, const uint4* __restrict__ best, const float2* __restrict__ qxy,
                                                       const float2* __restrict__ txy, int use_ratio, float r2, uint32_t max_distance,
                                                       int unique, const unsigned long long* __restrict__ tmin,
                                                       uint4* __restrict__ out, uint32_t* __restrict__ out_count) {
    const char* recs;
    const unsigned nq = list_resolve(Q, recs);
    const unsigned first = blockIdx.x * 256u + (threadIdx.x & ~63u);
    if (first >= nq) return;  // wave-uniform
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    bool keep = i < nq;
    uint4 b = make_uint4(kNone, kNone, kNone, 0u);
    if (keep) {
        b = best[i];
        keep = passes_ratio_and_cap(b.x, b.y, b.z, use_ratio, r2, max_distance);
    }
    if (keep && unique) keep = tmin[b.y] == (((unsigned long long)b.x << 32) | i);
    uint4 lo = make_uint4(0, 0, 0, 0), hi = lo;
    if (keep) {
        const float2 q = qxy[i], t = txy[b.y];
        lo = make_uint4(i, b.y, b.x, b.z);
        hi = make_uint4(__float_as_uint(q.x), __float_as_uint(q.y), __float_as_uint(t.x), __float_as_uint(t.y));
    }
    emit_match_record(keep, lo, hi, out, out_count);  // at most nq <= the query capacity records
}
