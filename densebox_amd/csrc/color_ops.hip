// NV12 frames in and out: dbx_nv12_to_rgb_batch and dbx_rgb_to_nv12_batch (one launch over a device table of frames, like the painters'),
// dbx_nv12_host (the same pixel functions on one host frame) and dbx_resize_cubic_batch_nv12 (the bicubic resize tile of
// resize_tile.hpp with a source policy that fetches Y, U, V and converts the tap).  No reference counterpart; include/densebox_hip.h
// states the semantics, tests/nv12_ref.py restates them in NumPy.  The conversions are integer; the resize's coefficient arithmetic
// must give the bits NumPy gives, so floating-point contraction is OFF in this file as in resize_ops.hip.
#pragma clang fp contract(off)
#include <vector>

#include "common.hpp"
#include "frame_tile.hpp"
#include "resize_tile.hpp"

#define NV_TW 128                    // a tile: 128 x 16 pixels; lanes 0..127 own 8 x 2 pixels each, all 256 move the RGB rows
#define NV_TH 16
#define NV_THREADS 256

static_assert(sizeof(dbx_nv12_frame) == 48 && offsetof(dbx_nv12_frame, rgb) == 16 && offsetof(dbx_nv12_frame, h) == 24 &&
              offsetof(dbx_nv12_frame, pitch_y) == 32 && offsetof(dbx_nv12_frame, pitch_rgb) == 40, "dbx_nv12_frame is 48 bytes");
static_assert(sizeof(dbx_nv12_params) == 16, "dbx_nv12_params is 16 bytes");
static_assert(sizeof(dbx_resize_job_nv12) == 88 && offsetof(dbx_resize_job_nv12, sh) == 24 && offsetof(dbx_resize_job_nv12, pad_value) == 64 &&
              offsetof(dbx_resize_job_nv12, dst_off) == 80, "dbx_resize_job_nv12 is 88 bytes");

// ---------------------------------------------------------------------------------------------------------------- the pixel rules
struct NvCoef { int ky, rv, gu, gv, bu, yr, yg, yb, ur, ug, ub, vr, vg, vb, yo, bgr; };

static const int NV_TO_RGB[4][5] = {{DBX_NV12_601_LIMITED_TO_RGB}, {DBX_NV12_601_FULL_TO_RGB}, {DBX_NV12_709_LIMITED_TO_RGB},
                                    {DBX_NV12_709_FULL_TO_RGB}};
static const int NV_FROM_RGB[4][9] = {{DBX_NV12_601_LIMITED_FROM_RGB}, {DBX_NV12_601_FULL_FROM_RGB}, {DBX_NV12_709_LIMITED_FROM_RGB},
                                      {DBX_NV12_709_FULL_FROM_RGB}};

static int nv_coef(const char* fn, const dbx_nv12_params* p, NvCoef* k) {
    DBX_REQUIRE(p, "%s: null params", fn);
    DBX_REQUIRE(p->standard == 601 || p->standard == 709, "%s: standard=%d must be 601 or 709", fn, p->standard);
    DBX_REQUIRE(p->range == 0 || p->range == 1, "%s: range=%d must be 0 (limited) or 1 (full)", fn, p->range);
    DBX_REQUIRE(p->order == 0 || p->order == 1, "%s: order=%d must be 0 (RGB) or 1 (BGR)", fn, p->order);
    const int v = (p->standard == 709 ? 2 : 0) + p->range;
    const int* t = NV_TO_RGB[v];
    const int* f = NV_FROM_RGB[v];
    k->ky = t[0]; k->rv = t[1]; k->gu = t[2]; k->gv = t[3]; k->bu = t[4];
    k->yr = f[0]; k->yg = f[1]; k->yb = f[2]; k->ur = f[3]; k->ug = f[4]; k->ub = f[5]; k->vr = f[6]; k->vg = f[7]; k->vb = f[8];
    k->yo = p->range == 0 ? 16 : 0;
    k->bgr = p->order;
    return DBX_OK;
}

__host__ __device__ static inline int nv_clip8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// One pixel to RGB: px[0..2] in the byte order of the interleaved image.  |ky*C| < 2^23 and every chroma term < 2^23: 32 bits hold.
__host__ __device__ static inline void nv_px_to_rgb(const NvCoef& k, int Y, int U, int V, int* px) {
    const int c = k.ky * (Y - k.yo) + 8192, d = U - 128, e = V - 128;
    const int r = nv_clip8((c + k.rv * e) >> 14), g = nv_clip8((c + k.gu * d + k.gv * e) >> 14), b = nv_clip8((c + k.bu * d) >> 14);
    px[0] = k.bgr ? b : r; px[1] = g; px[2] = k.bgr ? r : b;
}
__host__ __device__ static inline int nv_luma(const NvCoef& k, int r, int g, int b) {
    return nv_clip8(((k.yr * r + k.yg * g + k.yb * b + 8192) >> 14) + k.yo);
}
// the chroma of a 2 x 2 block from the sums of its four pixels (0..1020 each)
__host__ __device__ static inline void nv_chroma(const NvCoef& k, int rs, int gs, int bs, int& U, int& V) {
    U = nv_clip8(((k.ur * rs + k.ug * gs + k.ub * bs + 32768) >> 16) + 128);
    V = nv_clip8(((k.vr * rs + k.vg * gs + k.vb * bs + 32768) >> 16) + 128);
}

// a record the launches skip and dbx_nv12_host refuses
__host__ __device__ static inline bool nv_frame_ok(const dbx_nv12_frame& f) {
    return f.y && f.uv && f.rgb && f.h > 0 && f.w > 0 && !((f.h | f.w) & 1) && f.pitch_y >= f.w && f.pitch_uv >= f.w &&
           (long long)f.pitch_rgb >= 3ll * f.w;
}

// ---------------------------------------------------------------------------------------------------------------- the kernels
typedef const __attribute__((address_space(1))) u32x2* nv_gsrc2_t;
typedef const __attribute__((address_space(1))) unsigned int* nv_gsrc1_t;
typedef const __attribute__((address_space(1))) u32x4* nv_gsrc4_t;
typedef __attribute__((address_space(1))) u32x2* nv_gdst2_t;

// eight consecutive bytes of a Y or UV row in two registers; byte i is (w[i >> 2] >> 8 * (i & 3)) & 255
struct Nv8 {
    unsigned w[2];
    __device__ __forceinline__ int byte(int i) const { return (int)(w[i >> 2] >> (8 * (i & 3))) & 255; }
    __device__ __forceinline__ void set(int i, int v) { w[i >> 2] |= (unsigned)v << (8 * (i & 3)); }
};

// n bytes (even, 2..8) at p: one 8-byte word where the address allows, else two dwords, else -- and for n < 8 -- bytes
__device__ __forceinline__ Nv8 nv_load8(rsz_gsrc_t p, int n) {
    Nv8 v;
    v.w[0] = v.w[1] = 0u;
    const int a = (int)((size_t)p & 7);
    if (n == 8 && a == 0) {
        const u32x2 q = *reinterpret_cast<nv_gsrc2_t>(p);
        v.w[0] = q.x; v.w[1] = q.y;
    } else if (n == 8 && a == 4) {
        v.w[0] = reinterpret_cast<nv_gsrc1_t>(p)[0]; v.w[1] = reinterpret_cast<nv_gsrc1_t>(p)[1];
    } else {
#pragma unroll
        for (int i = 0; i < 8; ++i)
            if (i < n) v.set(i, p[i]);
    }
    return v;
}
__device__ __forceinline__ void nv_store8(rsz_gdst_t p, int n, const Nv8& v) {
    const int a = (int)((size_t)p & 7);
    if (n == 8 && a == 0) {
        u32x2 q;
        q.x = v.w[0]; q.y = v.w[1];
        *reinterpret_cast<nv_gdst2_t>(p) = q;
    } else if (n == 8 && a == 4) {
        reinterpret_cast<rsz_gdst1_t>(p)[0] = v.w[0]; reinterpret_cast<rsz_gdst1_t>(p)[1] = v.w[1];
    } else {
#pragma unroll
        for (int i = 0; i < 8; ++i)
            if (i < n) p[i] = (unsigned char)v.byte(i);
    }
}

// rsz_store_row's mirror: nb bytes of one row at g to LDS, byte b of the row to L[shift + b], shift = g & 15, by lanes q of 16: aligned
// 16-byte words where the whole word is inside the row, else its whole dwords, else bytes, so no byte outside [g, g + nb) is read.
__device__ __forceinline__ void nv_load_row(rsz_gsrc_t g, unsigned char* L, int nb, int q16) {
    const int shift = (int)((size_t)g & 15), end = shift + nb;
    const rsz_gsrc_t gw = g - shift;
    for (int k = q16; 16 * k < end; k += 16) {
        const int b0 = 16 * k;
        if (b0 >= shift && b0 + 16 <= end) {
            reinterpret_cast<u32x4*>(L)[k] = reinterpret_cast<nv_gsrc4_t>(gw)[k];
        } else {
            for (int j = b0; j < b0 + 16; j += 4) {
                if (j >= shift && j + 4 <= end) {
                    reinterpret_cast<unsigned int*>(L)[j >> 2] = reinterpret_cast<nv_gsrc1_t>(gw)[j >> 2];
                } else {
                    for (int q = j < shift ? shift : j; q < j + 4 && q < end; ++q) L[q] = gw[q];
                }
            }
        }
    }
}

#define NV_ROW (NV_TW * 3 + 16)      // an RGB tile row in LDS: its bytes after a shift of 0..15

// The tile of workgroup blockIdx.x of frame blockIdx.y; false -- for the whole workgroup -- when the record is skipped or the tile lies
// outside the frame.
__device__ __forceinline__ bool nv_open(const dbx_nv12_frame* frames, int tiles_x, int max_h, int max_w, dbx_nv12_frame& f, int& x0, int& y0) {
    f = frames[blockIdx.y];
    x0 = (int)(blockIdx.x % tiles_x) * NV_TW; y0 = (int)(blockIdx.x / tiles_x) * NV_TH;
    return nv_frame_ok(f) && f.h <= max_h && f.w <= max_w && x0 < f.w && y0 < f.h;
}

// NV12 -> RGB.  Lane t < 128 owns the 8 x 2 pixels at column 8 * (t & 15), row 2 * (t >> 4) of the tile: 8 bytes of two Y rows and the 8
// bytes of their UV row, each pair used for its 2 x 2 block; the 48 RGB bytes go to LDS.  Then 16 lanes per row store the row.
__global__ __launch_bounds__(NV_THREADS) void nv12_to_rgb_kernel(const dbx_nv12_frame* __restrict__ frames, int tiles_x, int max_h, int max_w,
                                                                 const NvCoef k) {
    __shared__ __attribute__((aligned(16))) unsigned char stage[NV_TH][NV_ROW];
    dbx_nv12_frame f;
    int x0, y0;
    if (!nv_open(frames, tiles_x, max_h, max_w, f, x0, y0)) return;                   // uniform
    const int tid = threadIdx.x;
    const rsz_gdst_t rgb = (rsz_gdst_t)f.rgb;
    if (tid < NV_TW / 8 * (NV_TH / 2)) {
        const int gx = tid & 15, by = tid >> 4, x = x0 + 8 * gx, y = y0 + 2 * by;
        if (x < f.w && y < f.h) {                                                      // h is even: row y + 1 exists
            const int n = min(8, f.w - x);                                             // w is even: n is
            const rsz_gsrc_t py = (rsz_gsrc_t)f.y + (size_t)y * f.pitch_y + x;
            const Nv8 ya = nv_load8(py, n), yb = nv_load8(py + f.pitch_y, n);
            const Nv8 uv = nv_load8((rsz_gsrc_t)f.uv + (size_t)(y >> 1) * f.pitch_uv + x, n);
            const size_t g0 = (size_t)(rgb + (size_t)y * f.pitch_rgb + (size_t)x0 * 3);
            unsigned char* L0 = stage[2 * by] + (int)(g0 & 15) + gx * 24;
            unsigned char* L1 = stage[2 * by + 1] + (int)((g0 + (size_t)f.pitch_rgb) & 15) + gx * 24;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                if (i >= n) continue;
                const int U = uv.byte(i & ~1), V = uv.byte(i | 1);
                int p0[3], p1[3];
                nv_px_to_rgb(k, ya.byte(i), U, V, p0);
                nv_px_to_rgb(k, yb.byte(i), U, V, p1);
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) { L0[3 * i + ch] = (unsigned char)p0[ch]; L1[3 * i + ch] = (unsigned char)p1[ch]; }
            }
        }
    }
    __syncthreads();
    const int r = tid >> 4, yy = y0 + r;
    if (yy >= f.h) return;
    rsz_store_row(rgb + (size_t)yy * f.pitch_rgb + (size_t)x0 * 3, stage[r], min(NV_TW, f.w - x0) * 3, tid & 15);
}

// RGB -> NV12: 16 lanes per row load the tile's RGB rows into LDS; lane t < 128 then makes the 16 Y bytes and the 4 UV pairs of its 8 x 2
// pixels and stores them as 8-byte words where the addresses allow.
__global__ __launch_bounds__(NV_THREADS) void rgb_to_nv12_kernel(const dbx_nv12_frame* __restrict__ frames, int tiles_x, int max_h, int max_w,
                                                                 const NvCoef k) {
    __shared__ __attribute__((aligned(16))) unsigned char stage[NV_TH][NV_ROW];
    dbx_nv12_frame f;
    int x0, y0;
    if (!nv_open(frames, tiles_x, max_h, max_w, f, x0, y0)) return;                   // uniform
    const int tid = threadIdx.x;
    const rsz_gsrc_t rgb = (rsz_gsrc_t)f.rgb;
    {
        const int r = tid >> 4, yy = y0 + r;
        if (yy < f.h) nv_load_row(rgb + (size_t)yy * f.pitch_rgb + (size_t)x0 * 3, stage[r], min(NV_TW, f.w - x0) * 3, tid & 15);
    }
    __syncthreads();
    if (tid >= NV_TW / 8 * (NV_TH / 2)) return;
    const int gx = tid & 15, by = tid >> 4, x = x0 + 8 * gx, y = y0 + 2 * by;
    if (x >= f.w || y >= f.h) return;
    const int n = min(8, f.w - x);
    const size_t g0 = (size_t)(rgb + (size_t)y * f.pitch_rgb + (size_t)x0 * 3);
    const unsigned char* L0 = stage[2 * by] + (int)(g0 & 15) + gx * 24;
    const unsigned char* L1 = stage[2 * by + 1] + (int)((g0 + (size_t)f.pitch_rgb) & 15) + gx * 24;
    const int ir = k.bgr ? 2 : 0, ib = 2 - ir;
    Nv8 ya, yb, uv;
    ya.w[0] = ya.w[1] = yb.w[0] = yb.w[1] = uv.w[0] = uv.w[1] = 0u;
#pragma unroll
    for (int j = 0; j < 8; j += 2) {
        if (j >= n) continue;
        int rs = 0, gs = 0, bs = 0;
#pragma unroll
        for (int i = j; i < j + 2; ++i) {
            const int r0 = L0[3 * i + ir], g0v = L0[3 * i + 1], b0 = L0[3 * i + ib];
            const int r1 = L1[3 * i + ir], g1v = L1[3 * i + 1], b1 = L1[3 * i + ib];
            ya.set(i, nv_luma(k, r0, g0v, b0));
            yb.set(i, nv_luma(k, r1, g1v, b1));
            rs += r0 + r1; gs += g0v + g1v; bs += b0 + b1;
        }
        int U, V;
        nv_chroma(k, rs, gs, bs, U, V);
        uv.set(j, U);
        uv.set(j + 1, V);
    }
    const rsz_gdst_t py = (rsz_gdst_t)f.y + (size_t)y * f.pitch_y + x;
    nv_store8(py, n, ya);
    nv_store8(py + f.pitch_y, n, yb);
    nv_store8((rsz_gdst_t)f.uv + (size_t)(y >> 1) * f.pitch_uv + x, n, uv);
}

// ---------------------------------------------------------------------------------------------------------------- the fused resize
// The NV12 surface as a source of resize_tile_body: a tap's column and row offsets are its ABSOLUTE source coordinates (strides of 1),
// so its chroma is indexed as the conversion indexes it whatever the crop's origin; fetch converts the tap once for its three channels.
struct RszSrcNv12 {
    static constexpr int C = 3;
    rsz_gsrc_t y, uv;
    int pitch_y, pitch_uv;
    NvCoef k;
    __device__ __forceinline__ int col_stride() const { return 1; }
    __device__ __forceinline__ int row_stride() const { return 1; }
    // yo * pitch_y + xo < sh * pitch_y <= 2^31 - 1, and the chroma offset likewise (checked by the entry point)
    __device__ __forceinline__ void fetch(int yo, int xo, int* px) const {
        const int c = (yo >> 1) * pitch_uv + (xo & ~1);
        nv_px_to_rgb(k, (int)y[yo * pitch_y + xo], (int)uv[c], (int)uv[c + 1], px);
    }
};

struct ResizeJobNv12Dev {               // device record of one job (112 bytes): the resize's own, src = the Y plane, row_bytes = pitch_y
    ResizeJobDev j;
    const unsigned char* uv;
    int pitch_uv, pad;
};
static_assert(sizeof(ResizeJobNv12Dev) == 112, "ResizeJobNv12Dev layout");

// resize_cubic_batch_u8_kernel's walk (resize_ops.hip): one workgroup per tile, its job found by a binary search of tile0
__global__ __launch_bounds__(RSZ_THREADS) void resize_cubic_batch_nv12_kernel(const ResizeJobNv12Dev* __restrict__ jobs,
                                                                              const int* __restrict__ tile0, int njobs, const NvCoef k) {
    const int t = blockIdx.x;
    int lo = 0, hi = njobs - 1;                        // the last job whose first tile is <= t (jobs always have tiles)
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (tile0[mid] <= t) lo = mid; else hi = mid - 1;
    }
    const ResizeJobNv12Dev* J = jobs + lo;
    const int tt = t - tile0[lo], tiles_x = J->j.tiles_x;
    const int x0 = (tt % tiles_x) * RSZ_TW, y0 = (tt / tiles_x) * RSZ_TH;
    RszSrcNv12 src;
    src.y = (rsz_gsrc_t)J->j.src; src.uv = (rsz_gsrc_t)J->uv; src.pitch_y = J->j.row_bytes; src.pitch_uv = J->pitch_uv; src.k = k;
    resize_tile_body(&J->j, J->j.dst, x0, y0, src);
}

// ---------------------------------------------------------------------------------------------------------------- entry points
static int nv_batch(const char* fn, bool to_rgb, const dbx_nv12_frame* frames, int32_t batch, int32_t max_h, int32_t max_w,
                    const dbx_nv12_params* params, void* stream) {
    DBX_REQUIRE(batch >= 0, "%s: batch=%d is negative", fn, batch);
    DBX_REQUIRE(max_h >= 1 && max_w >= 1, "%s: max_h=%d and max_w=%d must be positive", fn, max_h, max_w);
    NvCoef k;
    int rc = nv_coef(fn, params, &k);
    if (rc != DBX_OK) return rc;
    DBX_REQUIRE(frames, "%s: null frames", fn);
    dim3 grid;
    int tiles_x = 0;
    rc = tile_grid<NV_TW, NV_TH>(fn, max_h, max_w, batch, &grid, &tiles_x);
    if (rc != DBX_OK || batch == 0) return rc;
    if (to_rgb) hipLaunchKernelGGL(nv12_to_rgb_kernel, grid, dim3(NV_THREADS), 0, (hipStream_t)stream, frames, tiles_x, max_h, max_w, k);
    else hipLaunchKernelGGL(rgb_to_nv12_kernel, grid, dim3(NV_THREADS), 0, (hipStream_t)stream, frames, tiles_x, max_h, max_w, k);
    DBX_LAUNCH_CHECK();
    return DBX_OK;
}

extern "C" int dbx_nv12_to_rgb_batch(const dbx_nv12_frame* frames, int32_t batch, int32_t max_h, int32_t max_w, const dbx_nv12_params* params,
                                     void* stream) {
    return nv_batch("nv12_to_rgb_batch", true, frames, batch, max_h, max_w, params, stream);
}

extern "C" int dbx_rgb_to_nv12_batch(const dbx_nv12_frame* frames, int32_t batch, int32_t max_h, int32_t max_w, const dbx_nv12_params* params,
                                     void* stream) {
    return nv_batch("rgb_to_nv12_batch", false, frames, batch, max_h, max_w, params, stream);
}

extern "C" int dbx_nv12_host(const dbx_nv12_frame* frame, const dbx_nv12_params* params, int32_t direction) {
    const char* fn = "nv12_host";
    DBX_REQUIRE(frame, "%s: null frame", fn);
    NvCoef k;
    const int rc = nv_coef(fn, params, &k);
    if (rc != DBX_OK) return rc;
    DBX_REQUIRE(direction == 0 || direction == 1, "%s: direction=%d must be 0 (to RGB) or 1 (from RGB)", fn, direction);
    const dbx_nv12_frame f = *frame;
    DBX_REQUIRE(f.y && f.uv && f.rgb, "%s: null plane", fn);
    DBX_REQUIRE(f.h > 0 && f.w > 0 && !((f.h | f.w) & 1), "%s: a frame of %d x %d pixels is empty or odd", fn, f.w, f.h);
    DBX_REQUIRE(nv_frame_ok(f), "%s: a pitch (%d, %d, %d) is below its row of %d pixels", fn, f.pitch_y, f.pitch_uv, f.pitch_rgb, f.w);
    const int ir = k.bgr ? 2 : 0, ib = 2 - ir;
    for (int y = 0; y < f.h; y += 2)
        for (int x = 0; x < f.w; x += 2) {
            uint8_t* uv = f.uv + (size_t)(y >> 1) * f.pitch_uv + x;
            int rs = 0, gs = 0, bs = 0;
            for (int q = 0; q < 4; ++q) {
                const int yy = y + (q >> 1), xx = x + (q & 1);
                uint8_t* yp = f.y + (size_t)yy * f.pitch_y + xx;
                uint8_t* p = f.rgb + (size_t)yy * f.pitch_rgb + (size_t)xx * 3;
                if (direction == 0) {
                    int px[3];
                    nv_px_to_rgb(k, *yp, uv[0], uv[1], px);
                    p[0] = (uint8_t)px[0]; p[1] = (uint8_t)px[1]; p[2] = (uint8_t)px[2];
                } else {
                    *yp = (uint8_t)nv_luma(k, p[ir], p[1], p[ib]);
                    rs += p[ir]; gs += p[1]; bs += p[ib];
                }
            }
            if (direction == 1) {
                int U, V;
                nv_chroma(k, rs, gs, bs, U, V);
                uv[0] = (uint8_t)U; uv[1] = (uint8_t)V;
            }
        }
    return DBX_OK;
}

static int64_t nv_tile0_offset(int32_t njobs) { return (int64_t)njobs * (int64_t)sizeof(ResizeJobNv12Dev); }

extern "C" int64_t dbx_resize_batch_nv12_workspace_bytes(int32_t njobs) {
    if (njobs < 0) return -1;
    return (nv_tile0_offset(njobs) + 4 * ((int64_t)njobs + 1) + 255) / 256 * 256;
}

extern "C" int dbx_resize_cubic_batch_nv12(const dbx_resize_job_nv12* jobs, int32_t njobs, const dbx_nv12_params* params, uint8_t* dst,
                                           void* workspace, void* stream) {
    const char* fn = "resize_cubic_batch_nv12";
    DBX_REQUIRE(njobs >= 0, "%s: njobs=%d is negative", fn, njobs);
    NvCoef k;
    const int rc = nv_coef(fn, params, &k);
    if (rc != DBX_OK) return rc;
    if (njobs == 0) return DBX_OK;
    DBX_REQUIRE(jobs && dst && workspace, "%s: null argument", fn);
    std::vector<ResizeJobNv12Dev> rec(njobs);
    std::vector<int> tile0(njobs + 1);
    long long tiles = 0;
    for (int j = 0; j < njobs; ++j) {
        const dbx_resize_job_nv12& g = jobs[j];
        DBX_REQUIRE(g.y && g.uv, "%s: job %d has a null plane", fn, j);
        DBX_REQUIRE(g.sh > 0 && g.sw > 0 && g.cw > 0 && g.ch > 0 && g.dh > 0 && g.dw > 0,
                    "%s: job %d has a non-positive size (source %d x %d, crop %d x %d, destination %d x %d)", fn, j, g.sh, g.sw, g.ch, g.cw,
                    g.dh, g.dw);
        DBX_REQUIRE(!((g.sh | g.sw) & 1), "%s: job %d source %d x %d has an odd side", fn, j, g.sh, g.sw);
        DBX_REQUIRE(g.pitch_y >= g.sw && g.pitch_uv >= g.sw, "%s: job %d has a pitch (%d, %d) below its row of %d pixels", fn, j, g.pitch_y,
                    g.pitch_uv, g.sw);
        DBX_REQUIRE((int64_t)g.sh * g.pitch_y <= 0x7fffffffLL && (int64_t)(g.sh / 2) * g.pitch_uv <= 0x7fffffffLL,
                    "%s: job %d planes of %d rows of %d and %d bytes exceed 2^31 - 1 bytes", fn, j, g.sh, g.pitch_y, g.pitch_uv);
        DBX_REQUIRE(g.cx0 >= 0 && g.cy0 >= 0 && (int64_t)g.cx0 + g.cw <= g.sw && (int64_t)g.cy0 + g.ch <= g.sh,
                    "%s: job %d crop (%d, %d) + %d x %d lies outside its %d x %d image", fn, j, g.cx0, g.cy0, g.cw, g.ch, g.sw, g.sh);
        DBX_REQUIRE(g.pad_l >= 0 && g.pad_t >= 0 && g.pad_r >= 0 && g.pad_b >= 0, "%s: job %d has negative padding", fn, j);
        const int64_t vw = (int64_t)g.cw + g.pad_l + g.pad_r, vh = (int64_t)g.ch + g.pad_t + g.pad_b;
        DBX_REQUIRE(vw <= (1 << 30) && vh <= (1 << 30), "%s: job %d padded size %lld x %lld exceeds 2^30", fn, j, (long long)vh, (long long)vw);
        DBX_REQUIRE(g.pad_value >= 0 && g.pad_value <= 255, "%s: job %d pad_value=%d must be 0..255", fn, j, g.pad_value);
        DBX_REQUIRE(g.dst_off >= 0, "%s: job %d has a negative dst_off", fn, j);
        ResizeJobNv12Dev& R = rec[j];
        ResizeJobDev& r = R.j;
        r.src = g.y; r.dst = dst + g.dst_off;
        r.scale_x = (double)vw / (double)g.dw; r.scale_y = (double)vh / (double)g.dh;
        r.row_bytes = g.pitch_y;
        r.cx0 = g.cx0; r.cy0 = g.cy0; r.cw = g.cw; r.ch = g.ch; r.pad_l = g.pad_l; r.pad_t = g.pad_t; r.vw = (int)vw; r.vh = (int)vh;
        r.dh = g.dh; r.dw = g.dw; r.pad_value = g.pad_value;
        r.tiles_x = (g.dw + RSZ_TW - 1) / RSZ_TW;
        r.pad[0] = r.pad[1] = r.pad[2] = 0;
        R.uv = g.uv; R.pitch_uv = g.pitch_uv; R.pad = 0;
        tile0[j] = (int)tiles;
        tiles += (long long)r.tiles_x * ((g.dh + RSZ_TH - 1) / RSZ_TH);
        DBX_REQUIRE(tiles <= 0xffffffffLL / RSZ_THREADS, "%s: more than %lld tiles of %d x %d pixels", fn, 0xffffffffLL / RSZ_THREADS, RSZ_TH,
                    RSZ_TW);
    }
    tile0[njobs] = (int)tiles;
    // pageable host source: the copy has read both vectors when it returns, so they may go out of scope (and `jobs` be reused)
    unsigned char* ws = (unsigned char*)workspace;
    DBX_HIP(hipMemcpyAsync(ws, rec.data(), sizeof(ResizeJobNv12Dev) * njobs, hipMemcpyHostToDevice, (hipStream_t)stream));
    DBX_HIP(hipMemcpyAsync(ws + nv_tile0_offset(njobs), tile0.data(), sizeof(int) * (njobs + 1), hipMemcpyHostToDevice, (hipStream_t)stream));
    hipLaunchKernelGGL(resize_cubic_batch_nv12_kernel, dim3((unsigned)tiles), dim3(RSZ_THREADS), 0, (hipStream_t)stream,
                       (const ResizeJobNv12Dev*)ws, (const int*)(ws + nv_tile0_offset(njobs)), njobs, k);
    DBX_LAUNCH_CHECK();
    return DBX_OK;
}
