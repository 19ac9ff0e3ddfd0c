// Descriptor matching (extension; the rule is in include/gdp.h): the exact nearest and second-nearest
// train descriptor of every query descriptor, brute force on the i8 matrix cores.
//
//   dist(i, j) = nq_i + nt_j - 2 dot(i, j),   dot = sum (q - 128)(t - 128),   n = sum (. - 128)^2
//
// Bytes become signed by `^ 0x80`; the dot product is v_mfma_i32_32x32x32_i8's int32 result, so every
// distance is an exact integer and the result does not depend on tiling, chunking or wave timing.
//
// k_match_norm    one thread per descriptor: its norm, and its packed key base (below)
// k_match_nn      one wave per (tile of 32 queries, chunk of the train list): the wave keeps its
//                 queries' 128 bytes in 16 VGPRs as operand B, streams train tiles of 32 as operand A
//                 (every fragment one 16-byte load straight from the 176-byte record) and reduces the
//                 accumulator in registers: the query is the accumulator's column, i.e. the lane
// k_match_select  one thread per query: merges the chunks, applies the tests, compacts per wave
//
// The register reduction.  For one lane the query is fixed, so (dist, j) is ordered like
// (dist - nq_i, j).  With nq_i = 2a + p the accumulator starts at -a, which makes
//     key = kb_j - (acc << 10),   kb_j = ((nt_j + 1) << 9) | (j & 511)
// equal to ((dist - p + 1) << 9) | (j & 511): one unsigned word, at most (8323201 << 9) | 511 <
// 0xffffffff, whose order IS the rule's (distance, index) order inside an aligned window of 512 train
// records.  The smallest two keys of a window are kept with max + min + min per accumulator register;
// at every window end they are folded into the full (best distance, best index, second distance).

constexpr int kMaTile = 32;            // queries per wave; train records per MFMA tile
constexpr int kMaWaves = 4;            // waves (query tiles) per block of k_match_nn
constexpr int kMaBlock = 64 * kMaWaves;
constexpr int kMaChunkUnit = 128;      // a chunk of the other list is a multiple of this many records
constexpr int kMaWindow = 512;         // records per packed-key window (9 index bits)
constexpr int kMaTargetWaves = 4096;   // chunks are added until the capacity grid has this many waves
constexpr unsigned kMaRecord = 176, kMaDesc = 48;  // sizeof(gdp_keypoint_described), offsetof(desc)

typedef int ma_i32x4 __attribute__((ext_vector_type(4)));
typedef int ma_i32x16 __attribute__((ext_vector_type(16)));

// One side of a match: the caller's list, else the describe object's image (gdp_pairs.inc).  A type of
// its own, so that the kernels' symbols name the stage's list
struct MaSide : ListRef<const char*> {};

// (B, I, S) <- merge with (b, i, s) whose indices all lie ABOVE those already merged: a tie keeps B
__device__ __forceinline__ void ma_merge_after(uint32_t& B, uint32_t& I, uint32_t& S, uint32_t b, uint32_t i, uint32_t s) {
    if (b < B) {
        S = B < s ? B : s;
        B = b;
        I = i;
    } else {
        S = S < b ? S : b;
    }
}

__device__ __forceinline__ ma_i32x4 ma_load_frag(const char* p) {
    const uint4 v = *reinterpret_cast<const uint4*>(p);
    ma_i32x4 f;
    f.x = (int)(v.x ^ 0x80808080u);
    f.y = (int)(v.y ^ 0x80808080u);
    f.z = (int)(v.z ^ 0x80808080u);
    f.w = (int)(v.w ^ 0x80808080u);
    return f;
}

// blockIdx.y = side.  norm[j] = sum (desc[k] - 128)^2, kb[j] = ((norm + 1) << 9) | (j & 511).
__global__ __launch_bounds__(256) void k_match_norm(MaSide s0, MaSide s1, uint32_t* __restrict__ norm0, uint32_t* __restrict__ kb0,
                                                    uint32_t* __restrict__ norm1, uint32_t* __restrict__ kb1) {
    const bool second = blockIdx.y != 0;  // field by field: a selected struct would live in scratch
    const MaSide s = {{second ? s1.src : s0.src, second ? s1.src_count : s0.src_count, second ? s1.src_cap : s0.src_cap,
                       second ? s1.own : s0.own, second ? s1.own_count : s0.own_count}};
    uint32_t* norm = second ? norm1 : norm0;
    uint32_t* kb = second ? kb1 : kb0;
    const char* recs;
    const unsigned n = list_resolve(s, recs);
    const unsigned j = blockIdx.x * 256u + threadIdx.x;
    if (j >= n) return;
    const uint4* d = reinterpret_cast<const uint4*>(recs + (size_t)j * kMaRecord + kMaDesc);
    uint32_t sum = 0;
    for (int k = 0; k < 8; ++k) {
        const uint4 v = d[k];
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
        for (int t = 0; t < 4; ++t)
            for (int e = 0; e < 4; ++e) {
                const int x = (int)((w[t] >> (8 * e)) & 255u) - 128;
                sum += (uint32_t)(x * x);
            }
    }
    norm[j] = sum;
    kb[j] = ((sum + 1u) << 9) | (j & (kMaWindow - 1));
}

// blockIdx.x: kMaWaves query tiles, blockIdx.y: chunk of the train list.  `qnorm` and `tkb` are
// k_match_norm's arrays of the two sides (padded to a multiple of kMaTile; values past the list are
// never used).  part[chunk * qpad + i] = (best distance, best index, second distance, 0).
__global__ __launch_bounds__(kMaBlock) void k_match_nn(MaSide Q, MaSide T, const uint32_t* __restrict__ qnorm,
                                                       const uint32_t* __restrict__ tkb, uint4* __restrict__ part, unsigned qpad,
                                                       unsigned chunks) {
    const unsigned lane = threadIdx.x & 63u, r = lane & 31u, h = lane >> 5;
    const unsigned q0 = (blockIdx.x * kMaWaves + (threadIdx.x >> 6)) * kMaTile;
    const char *qrecs, *trecs;
    const unsigned nq = list_resolve(Q, qrecs), nt = list_resolve(T, trecs);
    if (q0 >= nq || nt == 0) return;  // wave-uniform: the grid is sized from the capacities
    const unsigned len = chunk_len(nt, chunks, kMaChunkUnit);
    const unsigned long long begin = (unsigned long long)blockIdx.y * len;
    if (begin >= nt) return;
    const unsigned t_begin = (unsigned)begin, t_end = nt - t_begin < len ? nt : t_begin + len;

    // the queries: lane (r, h) holds bytes 32 ks + 16 h .. + 15 of query q0 + r for ks = 0..3 — and
    // the train side is loaded the same way, so A and B agree on the byte of every K index
    const unsigned qi = q0 + r < nq ? q0 + r : nq - 1;  // clamped; a masked column's values are never stored
    const char* qp = qrecs + (size_t)qi * kMaRecord + kMaDesc + 16u * h;
    ma_i32x4 qf[4];
    for (int ks = 0; ks < 4; ++ks) qf[ks] = ma_load_frag(qp + 32 * ks);
    const uint32_t nqv = qnorm[qi], par = nqv & 1u;
    ma_i32x16 cinit;
    for (int e = 0; e < 16; ++e) cinit[e] = -(int)(nqv >> 1);

    uint32_t B = kNone, I = kNone, S = kNone;  // the full triple of this lane's rows
    uint32_t kb1 = kNone, kb2 = kNone;           // the smallest two keys of the current window

    ma_i32x4 tf[4];
    uint4 kbv[4];
    auto load_tile = [&](unsigned j0, ma_i32x4 (&f)[4], uint4 (&k)[4]) {
        const unsigned ti = j0 + r < nt ? j0 + r : nt - 1;  // clamped; a masked row's values are never used
        const char* tp = trecs + (size_t)ti * kMaRecord + kMaDesc + 16u * h;
        for (int ks = 0; ks < 4; ++ks) f[ks] = ma_load_frag(tp + 32 * ks);
        // accumulator register 4g + e of this lane is train row j0 + 8g + 4h + e
        for (int g = 0; g < 4; ++g) k[g] = *reinterpret_cast<const uint4*>(tkb + j0 + 8u * g + 4u * h);
    };
    // one tile: four MFMAs, then 16 keys per lane into the window's smallest two.  `masked` is the
    // list's last, partial tile: rows at or past t_end become "no candidate"
    auto sweep_tile = [&](unsigned j0, const ma_i32x4 (&f)[4], const uint4 (&k)[4], auto masked) {
        ma_i32x16 acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(f[0], qf[0], cinit, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(f[1], qf[1], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(f[2], qf[2], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(f[3], qf[3], acc, 0, 0, 0);
        for (int g = 0; g < 4; ++g) {
            const uint32_t kw[4] = {k[g].x, k[g].y, k[g].z, k[g].w};
            for (int e = 0; e < 4; ++e) {
                // kb - (acc << 10); |acc| < 2^22, so the 24-bit multiply is exact (the compiler emits a shift and a subtract)
                uint32_t key = (uint32_t)__mul24(acc[4 * g + e], -1024) + kw[e];
                if constexpr (decltype(masked)::value)
                    if (j0 + 8u * g + 4u * h + e >= t_end) key = kNone;
                const uint32_t hi = key > kb1 ? key : kb1;
                kb2 = kb2 < hi ? kb2 : hi;
                kb1 = kb1 < key ? kb1 : key;
            }
        }
    };
    auto fold_window = [&](unsigned j0) {  // the window's two keys into the full triple
        const uint32_t base = j0 & ~(uint32_t)(kMaWindow - 1);
        const uint32_t d1 = kb1 == kNone ? kNone : (kb1 >> 9) - 1u + par;
        const uint32_t d2 = kb2 == kNone ? kNone : (kb2 >> 9) - 1u + par;
        ma_merge_after(B, I, S, d1, base + (kb1 & (kMaWindow - 1)), d2);
        kb1 = kb2 = kNone;
    };
    load_tile(t_begin, tf, kbv);
    unsigned j0 = t_begin;
#pragma unroll 2
    for (; j0 + kMaTile < t_end; j0 += kMaTile) {  // whole tiles that have a successor
        ma_i32x4 nf[4];
        uint4 nk[4];
        load_tile(j0 + kMaTile, nf, nk);  // the next tile's loads fly under this tile's MFMAs
        sweep_tile(j0, tf, kbv, std::false_type{});
        if (((j0 + kMaTile) & (kMaWindow - 1)) == 0) fold_window(j0);
        for (int ks = 0; ks < 4; ++ks) {
            tf[ks] = nf[ks];
            kbv[ks] = nk[ks];
        }
    }
    if (t_end - j0 < (unsigned)kMaTile)  // the chunk's last tile: partial only at the list's end
        sweep_tile(j0, tf, kbv, std::true_type{});
    else
        sweep_tile(j0, tf, kbv, std::false_type{});
    fold_window(j0);
    // the two lane halves hold interleaved rows of the same query: the rule's full order decides
    const uint32_t oB = (uint32_t)__shfl_xor((int)B, 32), oI = (uint32_t)__shfl_xor((int)I, 32), oS = (uint32_t)__shfl_xor((int)S, 32);
    const bool mine = B < oB || (B == oB && I <= oI);
    const uint32_t lose = mine ? oB : B;
    uint32_t sec = S < oS ? S : oS;
    sec = sec < lose ? sec : lose;
    if (h == 0 && q0 + r < nq) part[(size_t)blockIdx.y * qpad + q0 + r] = make_uint4(mine ? B : oB, mine ? I : oI, sec, 0u);
}

// One thread per query.  `part`: k_match_nn's triples with the queries on the lanes (tchunks chunks
// of the train list); `mpart`: those of the swapped pass (qchunks chunks of the query list, pitch
// tpad), read only when `mutual`.
__global__ __launch_bounds__(256) void k_match_select(MaSide Q, MaSide T, const uint4* __restrict__ part, unsigned qpad,
                                                      unsigned tchunks, const uint4* __restrict__ mpart, unsigned tpad,
                                                      unsigned qchunks, int use_ratio, float r2, uint32_t max_distance, int mutual,
                                                      uint4* __restrict__ out, uint32_t* __restrict__ out_count) {
    const char *qrecs, *trecs;
    const unsigned nq = list_resolve(Q, qrecs), nt = list_resolve(T, trecs);
    const unsigned first = blockIdx.x * 256u + (threadIdx.x & ~63u);
    if (first >= nq || nt == 0) return;  // wave-uniform
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    bool keep = i < nq;
    uint32_t B = kNone, I = kNone, S = kNone;
    if (keep) {
        const unsigned len = chunk_len(nt, tchunks, kMaChunkUnit), used = (nt + len - 1) / len;
        for (unsigned c = 0; c < used; ++c) {  // ascending chunks hold ascending indices
            const uint4 p = part[(size_t)c * qpad + i];
            ma_merge_after(B, I, S, p.x, p.y, p.z);
        }
        keep = passes_ratio_and_cap(B, I, S, use_ratio, r2, max_distance) && I < nt;  // I < nt always holds: nt >= 1 gave every query a candidate
    }
    if (keep && mutual) {  // is i the nearest query of train I, ties to the lowest query?
        const unsigned len = chunk_len(nq, qchunks, kMaChunkUnit), used = (nq + len - 1) / len;
        uint32_t mB = kNone, mI = kNone, mS = kNone;
        for (unsigned c = 0; c < used; ++c) {
            const uint4 p = mpart[(size_t)c * tpad + I];
            ma_merge_after(mB, mI, mS, p.x, p.y, p.z);
        }
        keep = mI == i;
    }
    uint4 lo = make_uint4(0, 0, 0, 0), hi = lo;
    if (keep) {
        float qx, qy, tx, ty;
        record_xy(qrecs + (size_t)i * kMaRecord, qx, qy);
        record_xy(trecs + (size_t)I * kMaRecord, tx, ty);
        lo = make_uint4(i, I, B, S);
        hi = make_uint4(__float_as_uint(qx), __float_as_uint(qy), __float_as_uint(tx), __float_as_uint(ty));
    }
    emit_match_record(keep, lo, hi, out, out_count);  // at most nq <= the query capacity records
}
