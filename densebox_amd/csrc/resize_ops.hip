// Batched pad + bicubic resize of uint8 images (pad_img + cv2.resize(..., INTER_CUBIC), DenseBox.py:1282-1340, and the patch
// cutters' cv2.resize of a cropped window, process_plate.py:244-252).  OpenCV is not part of the reference tree (and not installed
// here), so the kernel restates the generic C path of its 8-bit INTER_CUBIC resize (resize.cpp): float coefficients with A = -0.75
// rounded to 11-bit fixed point, a replicate border, 32-bit integer accumulation, (acc + 2^21) >> 22.  The coefficient arithmetic
// must give the bits NumPy gives in float32 / float64, so floating-point contraction is OFF in this file.
#pragma clang fp contract(off)
#include "common.hpp"
#include "resize_tile.hpp"

#include <vector>

// One launch over all jobs (dbx_resize_cubic_batch_u8).  A tile is RSZ_TH rows x RSZ_TW columns of one job's destination and one
// workgroup; tile0[j] is the first tile of job j (a prefix of the per-job tile counts) and each workgroup finds its job by a binary
// search of tile0, as the batched warp does.
// The tile itself is resize_tile_body (resize_tile.hpp), which the patch cutter runs as well.
template <int C>
__global__ __launch_bounds__(RSZ_THREADS) void resize_cubic_batch_u8_kernel(const ResizeJobDev* __restrict__ jobs,
                                                                              const int* __restrict__ tile0, int njobs) {
    const int t = blockIdx.x;
    int lo = 0, hi = njobs - 1;                        // the last job whose first tile is <= t (jobs always have tiles)
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (tile0[mid] <= t) lo = mid; else hi = mid - 1;
    }
    const ResizeJobDev* J = jobs + lo;
    const int tt = t - tile0[lo], tiles_x = J->tiles_x;
    const int x0 = (tt % tiles_x) * RSZ_TW, y0 = (tt / tiles_x) * RSZ_TH;
    resize_tile_body(J, J->dst, x0, y0, RszSrcU8<C>(J));
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
