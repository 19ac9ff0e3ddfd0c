// Homography warp of an input image (extension; the rule is in include/gdp.h): every pixel of the
// destination frame is mapped through the 3 x 3 matrix into the source image and sampled bilinearly.
//
// k_warp_prepare    one thread: step 1 (the matrix of this direction, FP64 without a division for the
//                   adjugate) into the record, its counters zeroed
// k_warp            the hot path.  A wave owns an 8 x 32 tile of the destination frame, a lane four
//                   consecutive columns of one row (a block: 2 x 2 waves, 16 x 64): under a rotation
//                   the wave's source footprint stays a compact patch.  m[] comes through scalar loads,
//                   the sixteen gathers of a lane are issued before any is used, the destination frame
//                   is loaded and the output stored as one vector per lane.  A block sweeps several
//                   tiles (the grid is capped at eight blocks per CU) with `covered` / `sad` in
//                   registers; they leave as one 32-bit and one 64-bit integer atomicAdd per block
//
// Every float operation of the rule is written as one C++ operation; the library is built with
// -ffp-contract=off -fno-fast-math -fno-gpu-flush-denormals-to-zero, which is part of the rule, and
// float32 `/` is hipcc's correctly rounded division.

constexpr int kWpTileRows = 8;     // rows of a wave's tile
constexpr int kWpTileCols = 32;    // its columns
constexpr int kWpLanePixels = 4;   // consecutive columns per lane
constexpr int kWpBlockRows = 16, kWpBlockCols = 64;  // 2 x 2 wave tiles
constexpr int kWpMaxDim = 1 << 24; // (float)(W - 1) is exact up to here: step 6 rests on it

struct WarpGeom {
    const void* src;       // the source image's first pixel
    const void* dst;       // the destination frame's
    void* out;             // the output, dense rows of out_pitch elements
    size_t src_pitch, dst_pitch, out_pitch;  // in elements
    int Hs, Ws, Hd, Wd;
    float xmax, ymax;      // (float)(Ws - 1), (float)(Hs - 1)
    int32_t fill;
    unsigned blocks_x;     // 16 x 64 block tiles per tile row of the frame
    unsigned tiles;        // block tiles of the frame, row-major
    int dst_vec;           // the frame's rows take one vector load per lane (alignment, pitch % 4 == 0)
};

// Step 1.  `own` non-NULL: the caller's nine floats; else the fit's model record (`model`, 16 words).
__global__ void k_warp_prepare(const uint32_t* __restrict__ model, const float* __restrict__ own, int direction, uint32_t pixels,
                               gdp_warp_record* __restrict__ rec) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    float h[9], m[9];
    bool valid = own != nullptr || model[9] != kNone;  // kNone: the hypothesis k_ransac_select stores without a model
    load_model(model, own, h);
    for (int k = 0; k < 9; ++k) m[k] = h[k];
    if (valid && direction == 1) {
        double M[3][3], G[3][3];
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) M[r][c] = (double)h[3 * r + c];
        ra_adj(M, G);
        const double det = (M[0][0] * G[0][0] + M[0][1] * G[1][0]) + M[0][2] * G[2][0];
        double s = 0.0;
        bool nan = false;
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) {
                const double a = fabs(G[r][c]);
                nan = nan || G[r][c] != G[r][c];
                s = a > s ? a : s;  // a NaN never becomes s: `nan` remembers it
            }
        valid = !nan && s > 0.0 && s < __builtin_inf() && det == det && det != 0.0;
        if (valid) {
            int e;
            (void)frexp(s, &e);
            const bool flip = det < 0.0;
            for (int r = 0; r < 3; ++r)
                for (int c = 0; c < 3; ++c) {
                    const double g = ldexp(G[r][c], -e);
                    m[3 * r + c] = (float)(flip ? -g : g);
                }
        }
    }
    for (int k = 0; k < 9; ++k) rec->m[k] = valid ? m[k] : 0.0f;
    rec->model = valid ? 1u : 0u;
    rec->covered = 0u;
    rec->pixels = pixels;
    rec->sad = 0ull;
    rec->direction = (uint32_t)direction;
    rec->reserved = 0u;
}

template <bool U8>
__device__ __forceinline__ float wp_pixel(const void* base, size_t index) {
    if (U8) return (float)static_cast<const uint8_t*>(base)[index];
    return (float)static_cast<const int32_t*>(base)[index];  // int -> float, round to nearest even
}

// step 3's end: val -> the stored integer
template <bool U8>
__device__ __forceinline__ int32_t wp_round(float val) {
    const float q = rintf(val);
    if (U8) return q >= 255.0f ? 255 : q <= 0.0f ? 0 : (int32_t)q;
    return q >= 2147483648.0f ? INT32_MAX : q < -2147483648.0f ? INT32_MIN : (int32_t)q;
}

// A block takes 16 x 64 tiles of the frame, row-major, gridDim.x apart.  `mrec` is the record's first ten words (m[9],
// model), which this launch only reads; `covered` and `sad` are its two counters.
template <bool SrcU8, bool DstU8>
__global__ __launch_bounds__(256) void k_warp(WarpGeom g, const uint32_t* __restrict__ mrec, uint32_t* __restrict__ covered,
                                               unsigned long long* __restrict__ sad) {
    __shared__ unsigned long long red_sad[4];
    __shared__ uint32_t red_cov[4];
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const int32_t fill = SrcU8 ? (g.fill < 0 ? 0 : g.fill > 255 ? 255 : g.fill) : g.fill;
    const bool model = mrec[9] != 0u;  // wave-uniform: without a model nothing is loaded
    float m[9];
    for (int k = 0; k < 9; ++k) m[k] = __uint_as_float(mrec[k]);
    uint32_t cov_n = 0;
    unsigned long long sad_n = 0;
    // a block sweeps the tiles blockIdx.x, blockIdx.x + gridDim.x, ...: the blocks running together work on
    // neighbouring tiles, and the sums stay in registers until the block's one pair of atomics
    for (unsigned tile = blockIdx.x; tile < g.tiles; tile += gridDim.x) {
        const unsigned by = tile / g.blocks_x, bx = tile - by * g.blocks_x;
        const unsigned r = by * kWpBlockRows + (wave >> 1) * kWpTileRows + (lane >> 3);
        const unsigned c0 = bx * kWpBlockCols + (wave & 1u) * kWpTileCols + (lane & 7u) * kWpLanePixels;
        const bool row_in = r < (unsigned)g.Hd, lane_in = row_in && c0 < (unsigned)g.Wd;
        int32_t out[kWpLanePixels] = {fill, fill, fill, fill};

        if (model) {
            bool cov[kWpLanePixels];
            float sx[kWpLanePixels], sy[kWpLanePixels];
            const float y = (float)r;
            for (int k = 0; k < kWpLanePixels; ++k) {
                const float x = (float)(c0 + (unsigned)k);
                float u, v, w;
                project(m, x, y, u, v, w);
                sx[k] = u / w;
                sy[k] = v / w;
                // a NaN fails every comparison
                cov[k] = row_in && c0 + (unsigned)k < (unsigned)g.Wd && w > 0.0f && sx[k] >= 0.0f && sy[k] >= 0.0f &&
                         sx[k] <= g.xmax && sy[k] <= g.ymax;
            }
            const bool any = cov[0] || cov[1] || cov[2] || cov[3];
            if (__ballot(any) != 0ull) {  // wave-uniform: a tile without a covered pixel keeps its fill
                // the gathers: indices of an uncovered pixel are 0, so every address lies in the source
                size_t at[kWpLanePixels][4];
                float fx[kWpLanePixels], fy[kWpLanePixels];
                for (int k = 0; k < kWpLanePixels; ++k) {
                    const float x0f = floorf(sx[k]), y0f = floorf(sy[k]);
                    const int x0 = cov[k] ? (int)x0f : 0, y0 = cov[k] ? (int)y0f : 0;  // 0 <= x0 <= Ws - 1 when covered
                    const int x1 = x0 + 1 < g.Ws - 1 ? x0 + 1 : g.Ws - 1, y1 = y0 + 1 < g.Hs - 1 ? y0 + 1 : g.Hs - 1;
                    fx[k] = sx[k] - x0f;
                    fy[k] = sy[k] - y0f;
                    at[k][0] = (size_t)y0 * g.src_pitch + (size_t)x0;
                    at[k][1] = (size_t)y0 * g.src_pitch + (size_t)x1;
                    at[k][2] = (size_t)y1 * g.src_pitch + (size_t)x0;
                    at[k][3] = (size_t)y1 * g.src_pitch + (size_t)x1;
                }
                float p[kWpLanePixels][4];
                for (int k = 0; k < kWpLanePixels; ++k)
                    for (int j = 0; j < 4; ++j) p[k][j] = wp_pixel<SrcU8>(g.src, at[k][j]);
                // the destination frame's four pixels of this lane, read as integers
                long long d[kWpLanePixels] = {0, 0, 0, 0};
                if (lane_in) {
                    const size_t first = (size_t)r * g.dst_pitch + c0;
                    if (g.dst_vec && c0 + (unsigned)kWpLanePixels <= (unsigned)g.Wd) {
                        if (DstU8) {
                            const uchar4 q = *reinterpret_cast<const uchar4*>(static_cast<const uint8_t*>(g.dst) + first);
                            d[0] = q.x, d[1] = q.y, d[2] = q.z, d[3] = q.w;
                        } else {
                            const int4 q = *reinterpret_cast<const int4*>(static_cast<const int32_t*>(g.dst) + first);
                            d[0] = q.x, d[1] = q.y, d[2] = q.z, d[3] = q.w;
                        }
                    } else {
                        for (int k = 0; k < kWpLanePixels; ++k)
                            if (c0 + (unsigned)k < (unsigned)g.Wd)
                                d[k] = DstU8 ? (long long)static_cast<const uint8_t*>(g.dst)[first + k]
                                             : (long long)static_cast<const int32_t*>(g.dst)[first + k];
                    }
                }
                for (int k = 0; k < kWpLanePixels; ++k) {
                    const float top = p[k][0] + fx[k] * (p[k][1] - p[k][0]);
                    const float bot = p[k][2] + fx[k] * (p[k][3] - p[k][2]);
                    const float val = top + fy[k] * (bot - top);
                    const int32_t q = wp_round<SrcU8>(val);
                    if (cov[k]) {
                        out[k] = q;
                        const long long diff = (long long)q - d[k];
                        sad_n += (unsigned long long)(diff < 0 ? -diff : diff);
                        cov_n += 1u;
                    }
                }
            }
        }

        // c0 is a multiple of 4 below Wd and out_pitch is Wd rounded up to 4: the vector stays in its row
        if (lane_in) {
            const size_t first = (size_t)r * g.out_pitch + c0;
            if (SrcU8)
                *reinterpret_cast<uchar4*>(static_cast<uint8_t*>(g.out) + first) =
                    make_uchar4((unsigned char)out[0], (unsigned char)out[1], (unsigned char)out[2], (unsigned char)out[3]);
            else
                *reinterpret_cast<int4*>(static_cast<int32_t*>(g.out) + first) = make_int4(out[0], out[1], out[2], out[3]);
        }
    }

    // integer sums: across the wave by shuffles, across the block in LDS, one atomic pair per block
    for (int dlt = 32; dlt >= 1; dlt >>= 1) {
        cov_n += (uint32_t)__shfl_xor((int)cov_n, dlt);
        sad_n += (unsigned long long)__shfl_xor((long long)sad_n, dlt);
    }
    if (lane == 0) {
        red_cov[wave] = cov_n;
        red_sad[wave] = sad_n;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int w = 1; w < 4; ++w) {
        cov_n += red_cov[w];
        sad_n += red_sad[w];
    }
    if (cov_n != 0u) {
        atomicAdd(covered, cov_n);
        atomicAdd(sad, sad_n);
    }
}
