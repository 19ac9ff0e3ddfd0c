// Least-squares refit of the RANSAC homography over its inliers (extension; the rule is in include/gdp.h):
// the inlier coordinates, quantised to 1/256 px and centred on their integer centroid, are reduced to 24
// moment sums in exact signed 128-bit integers, so the normal equations do not depend on order, tiling or
// wave timing; one thread solves them in separately rounded float64; the candidate replaces the model when
// it accepts at least as many matches.  Per round, behind one memset of the accumulators:
//
// k_refit_origin    one record per thread and grid-stride step: four int64 sums and the used count
// k_refit_moments   the hot path, twice (12 sums each, so the accumulators stay in registers): per-thread
//                   __int128 accumulators, reduced across the wave by shuffling their four dwords, across the
//                   block through LDS, then 32-bit limbs added into 64-bit integer atomics
// k_refit_solve     one thread: the sums, the scale exponents, the 8 x 8 LDL^T solve, the candidate record
// k_refit_count     lane = match, both matrices uniform: one ballot and population count per model
// k_refit_decide    one thread: the acceptance, the model record, the inlier counter, the refit record
// k_refit_inliers   k_ransac_inliers' pattern under the accepted model, gated on the decision
//
// Every float operation of the rule is one C++ operation (-ffp-contract=off, as for gdp_ransac.inc).

constexpr int kRfPerBlock = 2048;   // records of the capacity per block of the grid-stride sweeps
constexpr int kRfMaxBlocks = 1024;  // so a limb accumulator holds < 2^12 blocks x 4 waves x 2^32 < 2^64
constexpr uint32_t kRfMaxRounds = 8;
constexpr float kRfLimit = 16384.0f;  // a coordinate is used when |f| < this: |q| < 2^22, |q - o| < 2^23

// gdp_refit_record.status
enum : uint32_t { kRfAccepted = 1, kRfTooFew = 2, kRfPivot = 3, kRfNonFinite = 4, kRfFewer = 5, kRfNoModel = 6 };

// Words of the refit's one allocation.  The call's memset zeroes all of it, a later round's only acc[].
constexpr size_t kRfRecWords = 24;                   // the gdp_refit_record
constexpr size_t kRfFlagWords = 4;                   // stop (a round rejected, or no model), accept (this round)
constexpr size_t kRfCandWords = 24;                  // status, kq, kt, used | skipped, 0, 0, 0 | origin[4] | h[9], 0, 0, 0
constexpr size_t kRfAccWords = 8 + 24 * 4;           // uint64: origin sums[4], used, 0, c_cur, c_new, then 24 sums x 4 limbs
constexpr size_t kRfBytes = 4 * (kRfRecWords + kRfFlagWords + kRfCandWords) + 8 * kRfAccWords;

struct RfState {
    uint32_t* rec;
    uint32_t* flags;
    uint32_t* cand;
    unsigned long long* acc;
};

// The inlier list as it stands: the fit object's own buffer and counter
struct RfList {
    const uint4* recs;
    const uint32_t* count;
    unsigned cap;
};

__device__ __forceinline__ unsigned rf_len(const RfList& L) {
    const uint32_t n = *L.count;
    return n < L.cap ? n : L.cap;
}

// nothing to do: an earlier round of this call rejected its candidate, or there is no model
__device__ __forceinline__ bool rf_idle(const uint32_t* __restrict__ model, const RfState& st) {
    return st.flags[0] != 0 || model[9] == kNone;
}

// step 1: the four coordinates in 1/256 px; false = the record is skipped
__device__ __forceinline__ bool rf_quantise(uint4 c, long long (&q)[4]) {
    const float f[4] = {__uint_as_float(c.x), __uint_as_float(c.y), __uint_as_float(c.z), __uint_as_float(c.w)};
    bool used = true;
    for (int k = 0; k < 4; ++k) {
        used = used && fabsf(f[k]) < kRfLimit;  // false for a NaN and an infinity
        q[k] = (long long)rintf(f[k] * 256.0f);  // exact product; ties cannot occur beyond it
    }
    return used;
}

// floor(a / b) for b > 0
__device__ __forceinline__ long long rf_floor_div(long long a, long long b) {
    const long long q = a / b;
    return (a % b != 0 && a < 0) ? q - 1 : q;
}

// step 2 from the origin pass's sums; used >= 4
__device__ __forceinline__ void rf_origin(const unsigned long long* __restrict__ acc, long long (&o)[4]) {
    const long long used = (long long)acc[4];
    for (int k = 0; k < 4; ++k) o[k] = rf_floor_div((long long)acc[k], used);
}

__device__ __forceinline__ __int128 rf_shfl_xor(__int128 v, int d) {
    const unsigned __int128 u = (unsigned __int128)v;
    const uint32_t w0 = (uint32_t)__shfl_xor((int)(uint32_t)u, d), w1 = (uint32_t)__shfl_xor((int)(uint32_t)(u >> 32), d),
                   w2 = (uint32_t)__shfl_xor((int)(uint32_t)(u >> 64), d), w3 = (uint32_t)__shfl_xor((int)(uint32_t)(u >> 96), d);
    return (__int128)(((unsigned __int128)w3 << 96) | ((unsigned __int128)w2 << 64) | ((unsigned __int128)w1 << 32) | w0);
}

__global__ __launch_bounds__(256) void k_refit_origin(RfList L, RfState st, const uint32_t* __restrict__ model) {
    if (rf_idle(model, st)) return;
    __shared__ long long part[4][5];
    const unsigned n = rf_len(L), stride = gridDim.x * 256u;
    long long s[5] = {0, 0, 0, 0, 0};
    for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < n; i += stride) {  // n <= 2^30, stride <= 2^18: no wrap
        long long q[4];
        if (rf_quantise(L.recs[2 * (size_t)i + 1], q)) {
            for (int k = 0; k < 4; ++k) s[k] += q[k];
            s[4] += 1;
        }
    }
    for (int k = 0; k < 5; ++k)
        for (int d = 32; d >= 1; d >>= 1) s[k] += __shfl_xor(s[k], d);
    if ((threadIdx.x & 63u) == 0)
        for (int k = 0; k < 5; ++k) part[threadIdx.x >> 6][k] = s[k];
    __syncthreads();
    if (threadIdx.x < 5) {
        const long long v = (part[0][threadIdx.x] + part[1][threadIdx.x]) + (part[2][threadIdx.x] + part[3][threadIdx.x]);
        if (v != 0) atomicAdd(st.acc + threadIdx.x, (unsigned long long)v);  // two's complement: the sum of the q may be negative
    }
}

// Sum s = 6 b + a is mono_a(cx, cy) * tmono_b(cX, cY), mono = 1, x, y, x^2, xy, y^2 and tmono = 1, X, Y,
// X^2 + Y^2; HALF 0 sums b = 0, 1 and HALF 1 sums b = 2, 3.  |c| < 2^23, so a mono is < 2^46, a tmono < 2^47
// and a term < 2^93; at most 2^30 terms.
template <int HALF>
__global__ __launch_bounds__(256) void k_refit_moments(RfList L, RfState st, const uint32_t* __restrict__ model) {
    if (rf_idle(model, st) || st.acc[4] < 4) return;  // uniform over the grid
    __shared__ alignas(16) uint32_t part[4][48];
    long long o[4];
    rf_origin(st.acc, o);
    const unsigned n = rf_len(L), stride = gridDim.x * 256u;
    __int128 s[12];
    for (int k = 0; k < 12; ++k) s[k] = 0;
    for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < n; i += stride) {
        long long q[4];
        if (!rf_quantise(L.recs[2 * (size_t)i + 1], q)) continue;
        const long long cx = q[0] - o[0], cy = q[1] - o[1], cX = q[2] - o[2], cY = q[3] - o[3];
        const long long mono[6] = {1, cx, cy, cx * cx, cx * cy, cy * cy};
        const long long t0 = HALF ? cY : 1, t1 = HALF ? cX * cX + cY * cY : cX;
        for (int a = 0; a < 6; ++a) {
            s[a] += (__int128)mono[a] * t0;
            s[6 + a] += (__int128)mono[a] * t1;
        }
    }
    for (int k = 0; k < 12; ++k)
        for (int d = 32; d >= 1; d >>= 1) s[k] += rf_shfl_xor(s[k], d);
    if ((threadIdx.x & 63u) == 0) {
        uint4* p = reinterpret_cast<uint4*>(part[threadIdx.x >> 6]);
        for (int k = 0; k < 12; ++k) {
            const unsigned __int128 u = (unsigned __int128)s[k];
            p[k] = make_uint4((uint32_t)u, (uint32_t)(u >> 32), (uint32_t)(u >> 64), (uint32_t)(u >> 96));
        }
    }
    __syncthreads();
    if (threadIdx.x < 48) {  // one limb of one sum: the top limb carries the sign
        const unsigned t = threadIdx.x;
        long long v = 0;
        for (int w = 0; w < 4; ++w) v += (t & 3u) == 3u ? (long long)(int32_t)part[w][t] : (long long)part[w][t];
        if (v != 0) atomicAdd(st.acc + 8 + 48 * HALF + t, (unsigned long long)v);
    }
}

// a 128-bit sum from its four limb accumulators, modulo 2^128 (the true value fits)
__device__ __forceinline__ __int128 rf_sum(const unsigned long long* __restrict__ limb) {
    return (__int128)((unsigned __int128)limb[0] + ((unsigned __int128)limb[1] << 32) + ((unsigned __int128)limb[2] << 64) +
                      ((unsigned __int128)limb[3] << 96));
}

// step 5's conversion: +-((double)hi64 * 2^64 + (double)lo64) of the magnitude, times 2^-shift
__device__ __forceinline__ double rf_to_double(__int128 v, int shift) {
    const bool neg = v < 0;
    const unsigned __int128 m = neg ? (unsigned __int128)0 - (unsigned __int128)v : (unsigned __int128)v;
    const double d = (double)(unsigned long long)(m >> 64) * 18446744073709551616.0 + (double)(unsigned long long)m;
    return ldexp(neg ? -d : d, -shift);
}

// step 4: the smallest k >= 0 with sum < used * 4^k (sum < 2^30 * 2^47, so k <= 24)
__device__ __forceinline__ int rf_scale(__int128 sum, unsigned long long used) {
    int k = 0;
    while (k < 32 && !(sum < ((__int128)used << (2 * k)))) ++k;
    return k;
}

__global__ __launch_bounds__(64) void k_refit_solve(RfList L, RfState st, const uint32_t* __restrict__ model) {
    if (threadIdx.x != 0 || rf_idle(model, st)) return;
    const unsigned long long* acc = st.acc;
    const uint32_t listed = rf_len(L), used = (uint32_t)acc[4];
    uint32_t status = 0, kq = 0, kt = 0;
    long long o[4] = {0, 0, 0, 0};
    float hf[9] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (used < 4) {
        status = kRfTooFew;
    } else {
        rf_origin(acc, o);
        kq = (uint32_t)rf_scale(rf_sum(acc + 8 + 4 * 3) + rf_sum(acc + 8 + 4 * 5), used);
        kt = (uint32_t)rf_scale(rf_sum(acc + 8 + 4 * 18), used);
        double S[24];
        for (int b = 0; b < 4; ++b)
            for (int a = 0; a < 6; ++a) {
                const int dq = a == 0 ? 0 : a < 3 ? 1 : 2, dt = b == 0 ? 0 : b < 3 ? 1 : 2;
                S[6 * b + a] = rf_to_double(rf_sum(acc + 8 + 4 * (6 * b + a)), (int)kq * dq + (int)kt * dt);
            }
        // the lower triangle of the normal matrix and the right-hand side, as the header lists them
        double N[8][8], rhs[8];
        for (int i = 0; i < 8; ++i)
            for (int j = 0; j < 8; ++j) N[i][j] = 0.0;
        const double P[3][3] = {{S[3], S[4], S[1]}, {S[4], S[5], S[2]}, {S[1], S[2], S[0]}};
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j <= i; ++j) N[i][j] = N[3 + i][3 + j] = P[i][j];
        for (int b = 1; b <= 2; ++b) {  // X against h0..h2, Y against h3..h5
            const double* T = S + 6 * b;
            const int c = 3 * (b - 1);
            N[6][c] = -T[3], N[6][c + 1] = -T[4], N[6][c + 2] = -T[1];
            N[7][c] = -T[4], N[7][c + 1] = -T[5], N[7][c + 2] = -T[2];
            rhs[c] = T[1], rhs[c + 1] = T[2], rhs[c + 2] = T[0];
        }
        N[6][6] = S[18 + 3], N[7][6] = S[18 + 4], N[7][7] = S[18 + 5];
        rhs[6] = -S[18 + 1], rhs[7] = -S[18 + 2];
        // LDL^T without pivoting
        double Lm[8][8], D[8], v[8];
        bool ok = true;
        for (int j = 0; j < 8 && ok; ++j) {
            for (int k = 0; k < j; ++k) v[k] = Lm[j][k] * D[k];
            double d = N[j][j];
            for (int k = 0; k < j; ++k) d = d - Lm[j][k] * v[k];
            D[j] = d;
            ok = d > 0.0;  // false for a NaN
            for (int i = j + 1; i < 8 && ok; ++i) {
                double e = N[i][j];
                for (int k = 0; k < j; ++k) e = e - Lm[i][k] * v[k];
                Lm[i][j] = e / d;
            }
        }
        if (!ok) {
            status = kRfPivot;
        } else {
            double z[8], h[8];
            for (int i = 0; i < 8; ++i) {
                double e = rhs[i];
                for (int k = 0; k < i; ++k) e = e - Lm[i][k] * z[k];
                z[i] = e;
            }
            for (int i = 7; i >= 0; --i) {
                double e = z[i] / D[i];
                for (int k = i + 1; k < 8; ++k) e = e - Lm[k][i] * h[k];
                h[i] = e;
            }
            // step 6: K = H^ Tq, G = Tt^-1 K
            const double a = ldexp(256.0, -(int)kq), bx = ldexp(-(double)o[0], -(int)kq), by = ldexp(-(double)o[1], -(int)kq);
            const double sc = ldexp(1.0, (int)kt - 8), tX = (double)o[2] / 256.0, tY = (double)o[3] / 256.0;
            const double Hh[3][3] = {{h[0], h[1], h[2]}, {h[3], h[4], h[5]}, {h[6], h[7], 1.0}};
            double K[3][3], G[3][3];
            for (int r = 0; r < 3; ++r) {
                K[r][0] = Hh[r][0] * a;
                K[r][1] = Hh[r][1] * a;
                K[r][2] = (Hh[r][0] * bx + Hh[r][1] * by) + Hh[r][2];
            }
            for (int c = 0; c < 3; ++c) {
                G[0][c] = sc * K[0][c] + tX * K[2][c];
                G[1][c] = sc * K[1][c] + tY * K[2][c];
                G[2][c] = K[2][c];
            }
            double s = 0.0;
            bool nan = false;
            for (int r = 0; r < 3; ++r)
                for (int c = 0; c < 3; ++c) {
                    const double g = fabs(G[r][c]);
                    nan = nan || g != g;
                    s = g > s ? g : s;
                }
            if (nan || !(s > 0.0 && s < __builtin_inf())) {
                status = kRfNonFinite;
            } else {
                int e;
                (void)frexp(s, &e);
                for (int r = 0; r < 3; ++r)
                    for (int c = 0; c < 3; ++c) hf[3 * r + c] = (float)ldexp(G[r][c], -e);
            }
        }
    }
    uint4* out = reinterpret_cast<uint4*>(st.cand);
    out[0] = make_uint4(status, kq, kt, used);
    out[1] = make_uint4(listed - used, 0u, 0u, 0u);
    out[2] = make_uint4((uint32_t)(int32_t)o[0], (uint32_t)(int32_t)o[1], (uint32_t)(int32_t)o[2], (uint32_t)(int32_t)o[3]);
    out[3] = make_uint4(__float_as_uint(hf[0]), __float_as_uint(hf[1]), __float_as_uint(hf[2]), __float_as_uint(hf[3]));
    out[4] = make_uint4(__float_as_uint(hf[4]), __float_as_uint(hf[5]), __float_as_uint(hf[6]), __float_as_uint(hf[7]));
    out[5] = make_uint4(__float_as_uint(hf[8]), 0u, 0u, 0u);
}

// The fit rule's step-5 counts of the model record and of the candidate (all 0 without one, so it counts
// nothing) over the match list.  The loop is wave-uniform.
__global__ __launch_bounds__(256) void k_refit_count(RaList M, float tt, RfState st, const uint32_t* __restrict__ model) {
    if (rf_idle(model, st)) return;
    const uint4* recs;
    const unsigned n = list_resolve(M, recs);
    float hc[9], hn[9];
    load_model(model, nullptr, hc);
    load_model(st.cand + 12, nullptr, hn);
    const unsigned lane = threadIdx.x & 63u, stride = gridDim.x * 256u;
    uint32_t cur = 0, cnd = 0;
    for (unsigned base = blockIdx.x * 256u + (threadIdx.x & ~63u); base < n; base += stride) {
        const unsigned i = base + lane;
        const bool in = i < n;
        const uint4 c = in ? recs[2 * (size_t)i + 1] : make_uint4(0u, 0u, 0u, 0u);
        const float x = __uint_as_float(c.x), y = __uint_as_float(c.y), X = __uint_as_float(c.z), Y = __uint_as_float(c.w);
        cur += (uint32_t)__popcll(__ballot(in && ra_inlier(hc, x, y, X, Y, tt)));
        cnd += (uint32_t)__popcll(__ballot(in && ra_inlier(hn, x, y, X, Y, tt)));
    }
    if (lane == 0) {
        if (cur) atomicAdd(st.acc + 6, (unsigned long long)cur);
        if (cnd) atomicAdd(st.acc + 7, (unsigned long long)cnd);
    }
}

// One thread.  Step 7's decision; on acceptance the model record takes the candidate and the inlier counter
// goes to 0 for k_refit_inliers.  The refit record is rewritten whole.
__global__ __launch_bounds__(64) void k_refit_decide(RaList M, RfState st, uint32_t* __restrict__ model, uint32_t* __restrict__ out_count,
                                                     uint32_t rounds, uint32_t round) {
    if (threadIdx.x != 0) return;
    st.flags[1] = 0;
    if (st.flags[0] != 0) return;
    uint4* rec = reinterpret_cast<uint4*>(st.rec);
    const uint4 zero = make_uint4(0u, 0u, 0u, 0u);
    if (model[9] == kNone) {
        rec[0] = make_uint4(rounds, 0u, 0u, 0u);
        rec[1] = make_uint4(0u, 0u, kRfNoModel, 0u);
        rec[2] = rec[3] = rec[4] = rec[5] = zero;
        st.flags[0] = 1;
        return;
    }
    const uint4* recs;
    const unsigned n = list_resolve(M, recs);
    const uint32_t* cand = st.cand;
    const uint32_t c_cur = (uint32_t)st.acc[6], c_new = (uint32_t)st.acc[7];
    const bool accept = cand[0] == 0 && c_new >= c_cur && c_new >= 4u;
    const uint32_t status = cand[0] != 0 ? cand[0] : accept ? kRfAccepted : kRfFewer;
    const uint32_t accepted = st.rec[1] + (accept ? 1u : 0u), before = round == 0 ? c_cur : st.rec[4];
    if (accept) {
        uint4* m = reinterpret_cast<uint4*>(model);
        const uint32_t hypothesis = model[9];
        m[0] = make_uint4(cand[12], cand[13], cand[14], cand[15]);
        m[1] = make_uint4(cand[16], cand[17], cand[18], cand[19]);
        m[2] = make_uint4(cand[20], hypothesis, c_new, n);
        *out_count = 0;
    }
    rec[0] = make_uint4(rounds, accepted, cand[3], cand[4]);                  // rounds, accepted, used, skipped
    rec[1] = make_uint4(before, accept ? c_new : model[10], status, cand[1]);  // count_before, count_after, status, kq
    rec[2] = make_uint4(cand[2], cand[8], cand[9], cand[10]);                 // kt, origin[0..2]
    rec[3] = make_uint4(cand[11], cand[12], cand[13], cand[14]);              // origin[3], h[0..2]
    rec[4] = make_uint4(cand[15], cand[16], cand[17], cand[18]);
    rec[5] = make_uint4(cand[19], cand[20], 0u, 0u);
    st.flags[0] = accept ? 0u : 1u;
    st.flags[1] = accept ? 1u : 0u;
}

// One thread per match; the grid is sized from the capacity.  Writes nothing unless this round accepted.
__global__ __launch_bounds__(256) void k_refit_inliers(RaList M, float tt, RfState st, const uint32_t* __restrict__ model,
                                                       uint4* __restrict__ out, uint32_t* __restrict__ out_count) {
    if (st.flags[1] == 0) return;
    const uint4* recs;
    const unsigned n = list_resolve(M, recs);
    const unsigned first = blockIdx.x * 256u + (threadIdx.x & ~63u);
    if (first >= n) return;  // wave-uniform
    float m[9];
    load_model(model, nullptr, m);
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
