// What the two-image stages share (gdp_match.inc, gdp_ransac.inc, gdp_warp.inc, gdp_guided.inc; the rules
// are in include/gdp.h): the input list a launch resolves, a list's chunk length, a described record's
// image coordinates, the ratio and cap tests, the per-wave compaction of match records, and the model's
// nine floats with their projection.  Each piece of the rule is here once; every float operation is one
// C++ operation (the library is built with -ffp-contract=off -fno-fast-math
// -fno-gpu-flush-denormals-to-zero, which is part of the rule).

// no candidate, no model, no list of the caller's: a key, a distance, an index, a cell, a d_in_count
constexpr uint32_t kNone = 0xffffffffu;

// A stage's input list: the caller's when its count is not kNone, else the first
// min(counter, both capacities) records of the producer's.  P addresses the records: const char* for
// the 176-byte described records, const uint4* for the 32-byte match records.
template <class P>
struct ListRef {
    P src;
    const uint32_t* src_count;
    unsigned src_cap;  // min(the producer's capacity, the consumer's)
    P own;
    const uint32_t* own_count;
};

template <class P>
__device__ __forceinline__ unsigned list_resolve(const ListRef<P>& s, P& recs) {
    const uint32_t own = *s.own_count;
    if (own != kNone) {
        recs = s.own;
        return own;
    }
    recs = s.src;
    const uint32_t n = *s.src_count;
    return n < s.src_cap ? n : s.src_cap;
}

// chunk length for a list of n records cut into at most `chunks` chunks, a multiple of `unit`: the same
// expression wherever a grid's y axis walks a list (and in tests/test_gpu_match.py, test_gpu_ransac.py)
__device__ __forceinline__ unsigned chunk_len(unsigned n, unsigned chunks, unsigned unit) {
    const unsigned per = (n + chunks - 1) / chunks;
    return (per + unit - 1) / unit * unit;
}

// step 7 of the match rule: a described record's image coordinates
__device__ __forceinline__ void record_xy(const char* rec, float& x, float& y) {
    const uint4* p = reinterpret_cast<const uint4*>(rec);
    const uint4 w0 = p[0], w1 = p[1];  // octave | scale | kind, row, col, value;  dscale, drow, dcol, interp
    const float sc = (float)(1u << (w0.x & 31u));
    x = ((float)(int)w0.z + __uint_as_float(w1.z)) * sc;
    y = ((float)(int)w0.y + __uint_as_float(w1.y)) * sc;
}

// steps 5 and 6 of the match rule on (best distance, best index, second distance): a candidate, the
// ratio test (one rounded product and one comparison; (float)0xffffffff is 2^32) and the cap
__device__ __forceinline__ bool passes_ratio_and_cap(uint32_t B, uint32_t I, uint32_t S, int use_ratio, float r2, uint32_t max_distance) {
    bool keep = I != kNone;
    if (use_ratio) keep = keep && __uint2float_rn(B) < r2 * __uint2float_rn(S);
    return keep && B <= max_distance;
}

// Compaction of 32-byte match records per wave: one ballot, one atomic, two 16-byte stores.  Every lane
// of the wave calls it; at most one record per thread of the grid, which the capacity sized, so the
// buffer cannot overflow.
__device__ __forceinline__ void emit_match_record(bool keep, uint4 lo, uint4 hi, uint4* __restrict__ out, uint32_t* __restrict__ out_count) {
    const unsigned long long mask = __ballot(keep);
    if (mask == 0) return;
    const unsigned lane = threadIdx.x & 63u;
    uint32_t slot = 0;
    if (lane == 0) slot = atomicAdd(out_count, (uint32_t)__popcll(mask));
    slot = (uint32_t)__shfl((int)slot, 0);
    if (keep) {
        slot += (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
        out[2 * (size_t)slot] = lo;
        out[2 * (size_t)slot + 1] = hi;
    }
}

// The nine floats a launch works under: the caller's (`own` non-NULL), else the first nine words of the
// fit's model record (all 0 when it holds no model)
__device__ __forceinline__ void load_model(const uint32_t* __restrict__ model, const float* __restrict__ own, float (&h)[9]) {
    for (int k = 0; k < 9; ++k) h[k] = own ? own[k] : __uint_as_float(model[k]);
}

// (u, v, w) = h (x, y, 1): three times two rounded products and two rounded sums
__device__ __forceinline__ void project(const float (&h)[9], float x, float y, float& u, float& v, float& w) {
    u = (h[0] * x + h[1] * y) + h[2];
    v = (h[3] * x + h[4] * y) + h[5];
    w = (h[6] * x + h[7] * y) + h[8];
}
