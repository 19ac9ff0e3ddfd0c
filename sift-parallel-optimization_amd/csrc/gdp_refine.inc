// gdp_refine.inc — Sub-pixel keypoint refinement on the current pyramid: k_refine.
// Part of libgdp's single translation unit: included by gdp.hip inside its anonymous namespace
// (after `#pragma clang fp contract(off)`, which therefore applies here too).  Not a header.

// gdp_refine_keypoints (gdp.h): Lowe's localisation step on the records of the context's keypoint
// list.  A 3-D quadratic is fitted to the DoG around the sample (central differences), the offset
// of its extremum is solved by Cramer's rule, the sample moves by one per axis while the offset
// exceeds half a sample, and the converged point passes |interp| > contrast and, when edge_ratio
// != 0, the edge test at the final sample.  Every operation is the separately rounded float32
// operation gdp.h writes down, in its order; the three divisions are IEEE-correct (plain `/`).
//
// One lane per input record, 256-thread blocks over batch x ceil(capacity / 256).  Latency-bound:
// a step is 19 dependent-address loads scattered over three levels, so they are all issued before
// the step's arithmetic.  Lanes that converged or were rejected idle under the loop's predicate.
// Survivors are compacted per wave as k_extrema does: ballot + mbcnt rank, one atomic per wave.
constexpr int kRfBlock = 256;

struct RfFit {
    float v, gc, gr, gs, hcc, hrr, hss, hrc, hsc, hsr;
};

// The 19 samples of the 3 x 3 x 3 neighbourhood the fit reads (the 8 corners are not used) and the
// derivatives of gdp.h.  q points at D[s][r][c]; `cols` / `lev` are the row and level pitches.
__device__ __forceinline__ RfFit rf_fit(const float* __restrict__ q, long long cols, long long lev) {
    const float v = q[0];
    const float c_p = q[1], c_m = q[-1];
    const float r_p = q[cols], r_m = q[-cols];
    const float s_p = q[lev], s_m = q[-lev];
    const float rp_cp = q[cols + 1], rp_cm = q[cols - 1], rm_cp = q[1 - cols], rm_cm = q[-cols - 1];
    const float sp_cp = q[lev + 1], sp_cm = q[lev - 1], sm_cp = q[1 - lev], sm_cm = q[-lev - 1];
    const float sp_rp = q[lev + cols], sp_rm = q[lev - cols], sm_rp = q[cols - lev], sm_rm = q[-lev - cols];
    __builtin_amdgcn_sched_barrier(0);  // the loads go out before the step's arithmetic
    RfFit f;
    f.v = v;
    f.gc = (c_p - c_m) * 0.5f;
    f.gr = (r_p - r_m) * 0.5f;
    f.gs = (s_p - s_m) * 0.5f;
    f.hcc = (c_p + c_m) - 2.0f * v;
    f.hrr = (r_p + r_m) - 2.0f * v;
    f.hss = (s_p + s_m) - 2.0f * v;
    f.hrc = ((rp_cp - rp_cm) - (rm_cp - rm_cm)) * 0.25f;
    f.hsc = ((sp_cp - sp_cm) - (sm_cp - sm_cm)) * 0.25f;
    f.hsr = ((sp_rp - sp_rm) - (sm_rp - sm_rm)) * 0.25f;
    return f;
}

__global__ void __launch_bounds__(kRfBlock) k_refine(const Geom* __restrict__ g, const float* __restrict__ pyr,
                                                     const uint4* __restrict__ recs_in,
                                                     const unsigned* __restrict__ count_in, uint4* __restrict__ recs_out,
                                                     unsigned* __restrict__ count_out, unsigned long long capacity,
                                                     unsigned blocks_per_img, float thr, float er) {
    const unsigned b = blockIdx.x / blocks_per_img;
    const unsigned long long first = (unsigned long long)(blockIdx.x - b * blocks_per_img) * kRfBlock;
    const unsigned long long n = min((unsigned long long)count_in[b], capacity);  // block-uniform
    if (first >= n) return;
    const unsigned long long i = first + threadIdx.x;

    // the record; one that does not name a candidate of this geometry is dropped, never dereferenced
    bool active = i < n;
    uint4 rec = {0u, 0u, 0u, 0u};
    if (active) rec = recs_in[(unsigned long long)b * capacity + i];
    const int o = (int)(rec.x & 0xffffu);
    int s = (int)((rec.x >> 16) & 0xffu);
    int r = (int)rec.y, c = (int)rec.z;
    active = active && o < g->O;
    int rows = 0, cols = 0;
    long long lev = 0;
    const float* D = pyr;
    if (active) {
        const OctGeom& og = g->oct[o];
        rows = og.rows;
        cols = og.cols;
        lev = og.lev_stride;
        D = pyr + (long long)b * g->pyr_stride + og.lev_off;
    }
    const int S = g->S;
    active = active && s >= 1 && s <= S && r >= 1 && r <= rows - 2 && c >= 1 && c <= cols - 2;

    bool keep = false;
    float v = 0.f, xs = 0.f, xr = 0.f, xc = 0.f, interp = 0.f;
    for (int step = 0; step < GDP_REFINE_MAX_STEPS; ++step) {
        if (__ballot(active) == 0) break;  // wave-uniform
        if (active) {
            const RfFit f = rf_fit(D + (long long)s * lev + (long long)r * cols + c, cols, lev);
            const float A = f.hrr * f.hss - f.hsr * f.hsr;
            const float B = f.hrc * f.hss - f.hsc * f.hsr;
            const float C = f.hrc * f.hsr - f.hsc * f.hrr;
            const float E = f.hcc * f.hss - f.hsc * f.hsc;
            const float Q = f.hcc * f.hsr - f.hrc * f.hsc;
            const float G = f.hcc * f.hrr - f.hrc * f.hrc;
            const float det = (f.hcc * A - f.hrc * B) + f.hsc * C;
            if (!(fabsf(det) > 0.0f)) {
                active = false;  // singular or NaN
            } else {
                xc = -(((A * f.gc - B * f.gr) + C * f.gs) / det);
                xr = -(((E * f.gr - B * f.gc) - Q * f.gs) / det);
                xs = -(((C * f.gc - Q * f.gr) + G * f.gs) / det);
                if (fabsf(xc) <= 0.5f && fabsf(xr) <= 0.5f && fabsf(xs) <= 0.5f) {
                    v = f.v;
                    interp = f.v + ((f.gc * xc + f.gr * xr) + f.gs * xs) * 0.5f;
                    keep = fabsf(interp) > thr;
                    if (er != 0.0f && keep) {
                        const float tr = f.hcc + f.hrr;
                        const float d2 = f.hcc * f.hrr - f.hrc * f.hrc;
                        keep = d2 > 0.0f && (tr * tr) * er < ((er + 1.0f) * (er + 1.0f)) * d2;
                    }
                    active = false;
                } else {
                    const int dc = (int)(xc > 0.5f) - (int)(xc < -0.5f);
                    const int dr = (int)(xr > 0.5f) - (int)(xr < -0.5f);
                    const int ds = (int)(xs > 0.5f) - (int)(xs < -0.5f);
                    c += dc;
                    r += dr;
                    s += ds;
                    // nothing moved: a NaN offset; otherwise the walk may have left the candidates
                    active = (dc | dr | ds) != 0 && s >= 1 && s <= S && r >= 1 && r <= rows - 2 && c >= 1 && c <= cols - 2;
                }
            }
        }
    }

    const unsigned long long mask = __ballot(keep);
    if (mask == 0) return;  // wave-uniform
    const unsigned rank = __builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
    unsigned base = 0;
    if ((threadIdx.x & 63u) == 0) base = atomicAdd(count_out + b, (unsigned)__popcll(mask));
    base = (unsigned)__builtin_amdgcn_readfirstlane((int)base);
    const unsigned long long slot = (unsigned long long)base + rank;
    if (keep && slot < capacity) {  // outputs never exceed inputs: the bound is a safety net
        uint4* out = recs_out + 2ull * ((unsigned long long)b * capacity + slot);
        out[0] = uint4{(rec.x & 0xff00ffffu) | ((unsigned)s << 16), (unsigned)r, (unsigned)c, __float_as_uint(v)};
        out[1] = uint4{__float_as_uint(xs), __float_as_uint(xr), __float_as_uint(xc), __float_as_uint(interp)};
    }
}
