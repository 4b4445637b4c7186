// Batched pad + bicubic resize of uint8 images (pad_img + cv2.resize(..., INTER_CUBIC), DenseBox.py:1282-1340, and the patch
// cutters' cv2.resize of a cropped window, process_plate.py:244-252).  OpenCV is not part of the reference tree (and not installed
// here), so the kernel restates the generic C path of its 8-bit INTER_CUBIC resize (resize.cpp): float coefficients with A = -0.75
// rounded to 11-bit fixed point, a replicate border, 32-bit integer accumulation, (acc + 2^21) >> 22.  The coefficient arithmetic
// must give the bits NumPy gives in float32 / float64, so floating-point contraction is OFF in this file.
#pragma clang fp contract(off)
#include "common.hpp"

#include <vector>

// One launch over all jobs (dbx_resize_cubic_batch_u8).  A tile is RSZ_TH rows x RSZ_TW columns of one job's destination and one
// workgroup; tile0[j] is the first tile of job j (a prefix of the per-job tile counts) and each workgroup finds its job by a binary
// search of tile0, as the batched warp does.
//   1. Tables: the first RSZ_TW threads make the four 16-bit coefficients and the four source byte offsets (or -1: padding) of
//      their column, the next RSZ_TH threads those of their row -- once per tile, in LDS, not per pixel or per channel.
//   2. Pixels: the 64 lanes of a wave make 64 CONSECUTIVE pixels of one destination row, so the byte gathers of one load
//      instruction lie in one source row within a span of 64 * scale_x pixels; each wave makes RSZ_TH / 4 rows.  The column table
//      sits in registers for all rows, the row table is a wave-uniform LDS read.  The bytes go to LDS, each tile row placed at the
//      offset its global address has inside a 16-byte word.
//   3. Stores: 16 lanes per tile row store the row's aligned 16-byte words; a word that is only partly inside the row (at most
//      the first and the last) falls back to its whole dwords, then to bytes, so no byte outside the job's block is written.
// Source and destination go through global-address-space pointers (global_load / global_store, not flat).
#define RSZ_THREADS 256
#define RSZ_TW 64
#define RSZ_TH 16
#define RSZ_COEF_BITS 11
typedef const __attribute__((address_space(1))) unsigned char* rsz_gsrc_t;
typedef __attribute__((address_space(1))) unsigned char* rsz_gdst_t;
typedef __attribute__((address_space(1))) u32x4* rsz_gdst4_t;
typedef __attribute__((address_space(1))) unsigned int* rsz_gdst1_t;

struct ResizeJobDev {                   // device record of one job (96 bytes)
    const unsigned char* src;
    unsigned char* dst;                 // dst + dst_off
    double scale_x, scale_y;            // vw / dw, vh / dh
    int row_bytes;                      // sw * c
    int cx0, cy0, cw, ch, pad_l, pad_t, vw, vh, dh, dw, pad_value, tiles_x, pad[3];
};
static_assert(sizeof(ResizeJobDev) == 96, "ResizeJobDev layout");

// Destination index d of an axis with vn virtual source samples: coefficients a[0..3] of the taps s-1 .. s+2 and, per tap, the byte
// offset of its sample along that axis (index clamped to [0, vn - 1], then moved into the crop: c0 + index - pad0, times stride) or
// -1 when the clamped index lies in the padding.
__device__ __forceinline__ void cubic_taps(int d, double scale, int vn, int pad0, int cn, int c0, int stride, short* a, int* off) {
    float f = (float)(((double)d + 0.5) * scale - 0.5);
    const int s = (int)floorf(f);
    f -= (float)s;
    const float A = -0.75f;
    float c[4];
    c[0] = ((A * (f + 1.0f) - 5.0f * A) * (f + 1.0f) + 8.0f * A) * (f + 1.0f) - 4.0f * A;
    c[1] = ((A + 2.0f) * f - (A + 3.0f)) * f * f + 1.0f;
    c[2] = ((A + 2.0f) * (1.0f - f) - (A + 3.0f)) * (1.0f - f) * (1.0f - f) + 1.0f;
    c[3] = 1.0f - c[0] - c[1] - c[2];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int q = (int)rintf(c[k] * (float)(1 << RSZ_COEF_BITS));             // nearest, ties to even; no sum correction
        a[k] = (short)(q < -32768 ? -32768 : (q > 32767 ? 32767 : q));
        int v = s - 1 + k;
        v = (v < 0 ? 0 : (v > vn - 1 ? vn - 1 : v)) - pad0;
        off[k] = (v < 0 || v >= cn) ? -1 : (c0 + v) * stride;
    }
}

template <int C>
__global__ __launch_bounds__(RSZ_THREADS) void resize_cubic_batch_u8_kernel(const ResizeJobDev* __restrict__ jobs,
                                                                              const int* __restrict__ tile0, int njobs) {
    constexpr int ROW = RSZ_TW * C + 16;               // a tile row in LDS: its bytes after a shift of 0..15
    __shared__ __attribute__((aligned(16))) unsigned char stage[RSZ_TH][ROW];
    __shared__ short col_a[RSZ_TW][4], row_a[RSZ_TH][4];
    __shared__ int col_o[RSZ_TW][4], row_o[RSZ_TH][4];
    const int t = blockIdx.x, tid = threadIdx.x;
    int lo = 0, hi = njobs - 1;                        // the last job whose first tile is <= t (jobs always have tiles)
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (tile0[mid] <= t) lo = mid; else hi = mid - 1;
    }
    const ResizeJobDev* J = jobs + lo;
    const int tt = t - tile0[lo], tiles_x = J->tiles_x;
    const int x0 = (tt % tiles_x) * RSZ_TW, y0 = (tt / tiles_x) * RSZ_TH;
    const int dh = J->dh, dw = J->dw;
    if (tid < RSZ_TW) {
        const int x = x0 + tid < dw ? x0 + tid : dw - 1;
        cubic_taps(x, J->scale_x, J->vw, J->pad_l, J->cw, J->cx0, C, col_a[tid], col_o[tid]);
    } else if (tid < RSZ_TW + RSZ_TH) {
        const int r = tid - RSZ_TW, y = y0 + r < dh ? y0 + r : dh - 1;
        cubic_taps(y, J->scale_y, J->vh, J->pad_t, J->ch, J->cy0, J->row_bytes, row_a[r], row_o[r]);
    }
    __syncthreads();
    const rsz_gdst_t dst = (rsz_gdst_t)J->dst;
    {
        const int lane = tid & 63, wave = tid >> 6, x = x0 + lane;
        const rsz_gsrc_t src = (rsz_gsrc_t)J->src;
        const int pv = J->pad_value;
        int a[4], xo[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) { a[k] = col_a[lane][k]; xo[k] = col_o[lane][k]; }
#pragma unroll
        for (int i = 0; i < RSZ_TH / 4; ++i) {
            const int r = wave * (RSZ_TH / 4) + i, y = y0 + r;
            if (y >= dh || x >= dw) continue;
            // |acc| <= 255 * (1.375 * 2048)^2 = 2.02e9 < 2^31: 1.375 is the largest absolute coefficient sum (at f = 0.5), and the
            // same bound holds for every partial sum, so 32 bits hold in any order of summation.
            int acc[C];
#pragma unroll
            for (int ch = 0; ch < C; ++ch) acc[ch] = 0;
#pragma unroll
            for (int ky = 0; ky < 4; ++ky) {
                const int b = row_a[r][ky], yo = row_o[r][ky];
                int h[C];
#pragma unroll
                for (int ch = 0; ch < C; ++ch) h[ch] = 0;
#pragma unroll
                for (int kx = 0; kx < 4; ++kx) {
                    const bool padded = (xo[kx] | yo) < 0;
#pragma unroll
                    for (int ch = 0; ch < C; ++ch) h[ch] += a[kx] * (padded ? pv : (int)src[yo + xo[kx] + ch]);
                }
#pragma unroll
                for (int ch = 0; ch < C; ++ch) acc[ch] += b * h[ch];
            }
            const int shift = (int)((size_t)(dst + ((long long)y * dw + x0) * C) & 15);
#pragma unroll
            for (int ch = 0; ch < C; ++ch) {
                const int v = (acc[ch] + (1 << (2 * RSZ_COEF_BITS - 1))) >> (2 * RSZ_COEF_BITS);       // arithmetic shift
                stage[r][shift + lane * C + ch] = (unsigned char)(v < 0 ? 0 : (v > 255 ? 255 : v));
            }
        }
    }
    __syncthreads();
    const int r = tid >> 4, y = y0 + r;
    if (y >= dh) return;
    const int nb = (dw - x0 < RSZ_TW ? dw - x0 : RSZ_TW) * C;
    const rsz_gdst_t g = dst + ((long long)y * dw + x0) * C;
    const int shift = (int)((size_t)g & 15), end = shift + nb;
    const rsz_gdst_t gw = g - shift;                   // 16-byte aligned; byte b of the row is gw[shift + b] = stage[r][shift + b]
    const unsigned char* L = stage[r];
    for (int k = tid & 15; 16 * k < end; k += 16) {
        const int b0 = 16 * k;
        if (b0 >= shift && b0 + 16 <= end) {
            reinterpret_cast<rsz_gdst4_t>(gw)[k] = reinterpret_cast<const u32x4*>(L)[k];
        } else {
            for (int j = b0; j < b0 + 16; j += 4) {
                if (j >= shift && j + 4 <= end) {
                    reinterpret_cast<rsz_gdst1_t>(gw)[j >> 2] = reinterpret_cast<const unsigned int*>(L)[j >> 2];
                } else {
                    for (int q = j < shift ? shift : j; q < j + 4 && q < end; ++q) gw[q] = L[q];
                }
            }
        }
    }
}

static int64_t resize_tile0_offset(int32_t njobs) { return (int64_t)njobs * (int64_t)sizeof(ResizeJobDev); }

extern "C" int64_t dbx_resize_batch_workspace_bytes(int32_t njobs) {
    if (njobs < 0) return -1;
    return (resize_tile0_offset(njobs) + 4 * ((int64_t)njobs + 1) + 255) / 256 * 256;
}

extern "C" int dbx_resize_cubic_batch_u8(const dbx_resize_job* jobs, int32_t njobs, int32_t c, uint8_t* dst, void* workspace,
                                         void* stream) {
    DBX_REQUIRE(njobs >= 0, "resize_cubic_batch: njobs=%d is negative", njobs);
    DBX_REQUIRE(c >= 1 && c <= 4, "resize_cubic_batch: c=%d must be 1..4", c);
    if (njobs == 0) return DBX_OK;
    DBX_REQUIRE(jobs && dst && workspace, "resize_cubic_batch: null argument");
    std::vector<ResizeJobDev> rec(njobs);
    std::vector<int> tile0(njobs + 1);
    long long tiles = 0;
    for (int j = 0; j < njobs; ++j) {
        const dbx_resize_job& g = jobs[j];
        DBX_REQUIRE(g.src, "resize_cubic_batch: job %d has a null source", j);
        DBX_REQUIRE(g.sh > 0 && g.sw > 0 && g.cw > 0 && g.ch > 0 && g.dh > 0 && g.dw > 0,
                    "resize_cubic_batch: job %d has a non-positive size (source %d x %d, crop %d x %d, destination %d x %d)", j, g.sh,
                    g.sw, g.ch, g.cw, g.dh, g.dw);
        DBX_REQUIRE((int64_t)g.sh * g.sw * c <= 0x7fffffffLL, "resize_cubic_batch: job %d source %d x %d x %d exceeds 2^31 - 1 bytes", j,
                    g.sh, g.sw, c);
        DBX_REQUIRE(g.cx0 >= 0 && g.cy0 >= 0 && (int64_t)g.cx0 + g.cw <= g.sw && (int64_t)g.cy0 + g.ch <= g.sh,
                    "resize_cubic_batch: job %d crop (%d, %d) + %d x %d lies outside its %d x %d image", j, g.cx0, g.cy0, g.cw, g.ch, g.sw,
                    g.sh);
        DBX_REQUIRE(g.pad_l >= 0 && g.pad_t >= 0 && g.pad_r >= 0 && g.pad_b >= 0, "resize_cubic_batch: job %d has negative padding", j);
        const int64_t vw = (int64_t)g.cw + g.pad_l + g.pad_r, vh = (int64_t)g.ch + g.pad_t + g.pad_b;
        DBX_REQUIRE(vw <= (1 << 30) && vh <= (1 << 30), "resize_cubic_batch: job %d padded size %lld x %lld exceeds 2^30", j,
                    (long long)vh, (long long)vw);
        DBX_REQUIRE(g.pad_value >= 0 && g.pad_value <= 255, "resize_cubic_batch: job %d pad_value=%d must be 0..255", j, g.pad_value);
        DBX_REQUIRE(g.dst_off >= 0, "resize_cubic_batch: job %d has a negative dst_off", j);
        ResizeJobDev& r = rec[j];
        r.src = g.src; r.dst = dst + g.dst_off;
        r.scale_x = (double)vw / (double)g.dw; r.scale_y = (double)vh / (double)g.dh;
        r.row_bytes = g.sw * c;
        r.cx0 = g.cx0; r.cy0 = g.cy0; r.cw = g.cw; r.ch = g.ch; r.pad_l = g.pad_l; r.pad_t = g.pad_t; r.vw = (int)vw; r.vh = (int)vh;
        r.dh = g.dh; r.dw = g.dw; r.pad_value = g.pad_value;
        r.tiles_x = (g.dw + RSZ_TW - 1) / RSZ_TW;
        r.pad[0] = r.pad[1] = r.pad[2] = 0;
        tile0[j] = (int)tiles;
        tiles += (long long)r.tiles_x * ((g.dh + RSZ_TH - 1) / RSZ_TH);
        // one workgroup per tile, and a grid holds at most 2^32 - 1 work-items per dimension
        DBX_REQUIRE(tiles <= 0xffffffffLL / RSZ_THREADS, "resize_cubic_batch: more than %lld tiles of %d x %d pixels",
                    0xffffffffLL / RSZ_THREADS, RSZ_TH, RSZ_TW);
    }
    tile0[njobs] = (int)tiles;
    // pageable host source: the copy has read both vectors when it returns, so they may go out of scope (and `jobs` be reused)
    unsigned char* ws = (unsigned char*)workspace;
    DBX_HIP(hipMemcpyAsync(ws, rec.data(), sizeof(ResizeJobDev) * njobs, hipMemcpyHostToDevice, (hipStream_t)stream));
    DBX_HIP(hipMemcpyAsync(ws + resize_tile0_offset(njobs), tile0.data(), sizeof(int) * (njobs + 1), hipMemcpyHostToDevice,
                           (hipStream_t)stream));
    const ResizeJobDev* dj = (const ResizeJobDev*)ws;
    const int* dt = (const int*)(ws + resize_tile0_offset(njobs));
    const dim3 grid((unsigned)tiles), block(RSZ_THREADS);
    switch (c) {
        case 1: hipLaunchKernelGGL(resize_cubic_batch_u8_kernel<1>, grid, block, 0, (hipStream_t)stream, dj, dt, njobs); break;
        case 2: hipLaunchKernelGGL(resize_cubic_batch_u8_kernel<2>, grid, block, 0, (hipStream_t)stream, dj, dt, njobs); break;
        case 3: hipLaunchKernelGGL(resize_cubic_batch_u8_kernel<3>, grid, block, 0, (hipStream_t)stream, dj, dt, njobs); break;
        default: hipLaunchKernelGGL(resize_cubic_batch_u8_kernel<4>, grid, block, 0, (hipStream_t)stream, dj, dt, njobs); break;
    }
    DBX_LAUNCH_CHECK();
    return DBX_OK;
}
